// cos(2 pi i / 64), i = 0..63, as doubles: the values emrifd_host.cpp's CosTable holds (std::cos of
// the double 2 pi i / 64), written as hex floats so that the device reads the same bits.
// tests/test_traj_device_abi.py holds this table to them.
    0x1.0000000000000p+0, 0x1.fd88da3d12526p-1, 0x1.f6297cff75cb0p-1, 0x1.e9f4156c62ddap-1,
    0x1.d906bcf328d46p-1, 0x1.c38b2f180bdb1p-1, 0x1.a9b66290ea1a3p-1, 0x1.8bc806b151741p-1,
    0x1.6a09e667f3bcdp-1, 0x1.44cf325091dd6p-1, 0x1.1c73b39ae68c9p-1, 0x1.e2b5d3806f63ep-2,
    0x1.87de2a6aea964p-2, 0x1.294062ed59f05p-2, 0x1.8f8b83c69a60dp-3, 0x1.917a6bc29b438p-4,
    0x1.1a62633145c07p-54, -0x1.917a6bc29b42fp-4, -0x1.8f8b83c69a608p-3, -0x1.294062ed59f02p-2,
    -0x1.87de2a6aea962p-2, -0x1.e2b5d3806f63cp-2, -0x1.1c73b39ae68c6p-1, -0x1.44cf325091dd5p-1,
    -0x1.6a09e667f3bccp-1, -0x1.8bc806b151741p-1, -0x1.a9b66290ea1a4p-1, -0x1.c38b2f180bdb0p-1,
    -0x1.d906bcf328d46p-1, -0x1.e9f4156c62ddap-1, -0x1.f6297cff75cb0p-1, -0x1.fd88da3d12525p-1,
    -0x1.0000000000000p+0, -0x1.fd88da3d12526p-1, -0x1.f6297cff75cb0p-1, -0x1.e9f4156c62ddbp-1,
    -0x1.d906bcf328d47p-1, -0x1.c38b2f180bdb1p-1, -0x1.a9b66290ea1a5p-1, -0x1.8bc806b151742p-1,
    -0x1.6a09e667f3bcep-1, -0x1.44cf325091ddap-1, -0x1.1c73b39ae68c8p-1, -0x1.e2b5d3806f63fp-2,
    -0x1.87de2a6aea96dp-2, -0x1.294062ed59f07p-2, -0x1.8f8b83c69a619p-3, -0x1.917a6bc29b421p-4,
    -0x1.a79394c9e8a0ap-53, 0x1.917a6bc29b407p-4, 0x1.8f8b83c69a60cp-3, 0x1.294062ed59f00p-2,
    0x1.87de2a6aea967p-2, 0x1.e2b5d3806f63ap-2, 0x1.1c73b39ae68c5p-1, 0x1.44cf325091dd7p-1,
    0x1.6a09e667f3bcbp-1, 0x1.8bc806b15173ep-1, 0x1.a9b66290ea1a3p-1, 0x1.c38b2f180bdafp-1,
    0x1.d906bcf328d44p-1, 0x1.e9f4156c62ddap-1, 0x1.f6297cff75cafp-1, 0x1.fd88da3d12526p-1,
