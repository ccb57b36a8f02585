"""efd_stage_batch (host C, no GPU): the batched likelihood's packing of walker inputs.

Each walker's ten arrays must land 256-B aligned, in order, byte-exact in the staging buffer,
and its argument struct must carry the template's grid fields, its own nt, K and scale, and
dev_base + the array's offset; a short buffer is refused with the size it needs.
"""

import ctypes

import numpy as np
import pytest

from emri_frequencydomainwaveforms_amd import _lib
from emri_frequencydomainwaveforms_amd.summation import HOST_KEYS, BatchPreparer
from tests.helpers import source_inputs


def _walker(rng, nt, K):
    f = lambda n: rng.standard_normal(n)  # noqa: E731
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)  # noqa: E731
    return [f(nt), f(nt), f(nt), f(nt), f(nt), c(nt, K),
            rng.integers(-10, 10, K).astype(np.int32), rng.integers(-30, 30, K).astype(np.int32),
            c(K), c(K)]


def test_stage_batch_layout_and_args():
    lib = _lib.load()
    rng = np.random.default_rng(0)
    shapes = [(7, 3), (130, 41), (2, 1)]
    walkers = [_walker(rng, nt, K) for nt, K in shapes]
    src = np.array([[a.ctypes.data for a in w] for w in walkers], dtype=np.uint64)
    shape = np.array(shapes, dtype=np.int32)
    scale = np.array([[1.5, -0.25], [2.0, 0.0], [-1.0, 3.0]])
    tmpl = _lib.ModesumArgs(freq=0x1234, nf=999, grid_symmetric=1, caustic=1, k0=499)
    args = (_lib.ModesumArgs * 3)()
    total = ctypes.c_size_t(0)
    base = 1 << 40
    assert lib.efd_stage_batch(None, 0, base, 3, src.ctypes.data, shape.ctypes.data,
                               scale.ctypes.data, ctypes.byref(tmpl), args,
                               ctypes.byref(total)) == _lib.EFD_ERR_WORKSPACE
    need = total.value
    pin = np.zeros(need + 256, dtype=np.uint8)
    assert lib.efd_stage_batch(pin.ctypes.data, need - 1, base, 3, src.ctypes.data,
                               shape.ctypes.data, scale.ctypes.data, ctypes.byref(tmpl), args,
                               ctypes.byref(total)) == _lib.EFD_ERR_WORKSPACE
    assert lib.efd_stage_batch(pin.ctypes.data, pin.nbytes, base, 3, src.ctypes.data,
                               shape.ctypes.data, scale.ctypes.data, ctypes.byref(tmpl), args,
                               ctypes.byref(total)) == _lib.EFD_OK
    off = 0
    names = ("t", "phi_phi", "phi_r", "f_phi", "f_r", "amp", "m", "n", "ylm_p", "ylm_m")
    for i, w in enumerate(walkers):
        a = args[i]
        assert (a.nt, a.K) == shapes[i]
        assert (a.scale_re, a.scale_im) == tuple(scale[i])
        assert (a.freq, a.nf, a.grid_symmetric, a.caustic, a.k0) == (0x1234, 999, 1, 1, 499)
        for name, arr in zip(names, w):
            assert getattr(a, name) == base + off
            assert off % 256 == 0
            np.testing.assert_array_equal(pin[off:off + arr.nbytes], arr.reshape(-1).view(np.uint8))
            off = (off + arr.nbytes + 255) // 256 * 256
    assert off == need


@pytest.fixture(scope="module")
def hosts():
    """tests/test_gpu_batch_prepare.py's six ragged sources as BatchPreparer.submit's dicts."""
    return [{k: (np.ascontiguousarray(d[k].T) if k == "amp" else d[k]) for k in HOST_KEYS}
            for d in (source_inputs(M=M, e0=e0, T=0.02, dt=20.0, eps=eps)
                      for M, e0, eps in ((3e5, 0.35, 1e-2), (5e5, 0.2, 1e-3), (2e5, 0.5, 1e-2),
                                         (4e5, 0.1, 1e-5), (3e5, 0.6, 1e-2), (6e5, 0.3, 1e-4)))]


def _packed(h, alive):
    """The native upstream's form of a walker (waveform.py's prepare): the ten arrays' addresses
    and (nt, K) as bytes; the arrays themselves go to `alive`."""
    dts = (np.float64,) * 5 + (np.complex128, np.int32, np.int32, np.complex128, np.complex128)
    arrs = [np.ascontiguousarray(h[k], dtype=dt) for k, dt in zip(HOST_KEYS, dts)]
    alive.append(arrs)
    return {"_src": np.array([a.ctypes.data for a in arrs], dtype=np.uint64).tobytes(),
            "_shape": np.array(arrs[5].shape, dtype=np.int32).tobytes()}


def _staged(walkers):
    """(pinned buffer's bytes, argument structs' bytes) of the walkers through
    BatchPreparer._sources and efd_stage_batch."""
    lib = _lib.load()
    n = len(walkers)
    pend = [(h, None, True, complex(1.0 + i, -0.5 * i), 7, False) for i, h in enumerate(walkers)]
    src, shape, scale, keep = BatchPreparer._sources(pend)
    tmpl = _lib.ModesumArgs(freq=0x1234, nf=999, grid_symmetric=1, caustic=1, k0=7)
    args = (_lib.ModesumArgs * n)()
    total = ctypes.c_size_t(0)
    call = lambda pin, nbytes: lib.efd_stage_batch(  # noqa: E731
        pin, nbytes, 1 << 40, n, src.ctypes.data, shape.ctypes.data, scale.ctypes.data,
        ctypes.byref(tmpl), args, ctypes.byref(total))
    assert call(None, 0) == _lib.EFD_ERR_WORKSPACE
    pin = np.zeros(total.value, dtype=np.uint8)
    assert call(pin.ctypes.data, pin.nbytes) == _lib.EFD_OK
    del keep
    return pin, ctypes.string_at(args, ctypes.sizeof(args))


def test_sources_mixed_and_packed_walkers_stage_the_same_bytes(hosts):
    """A group mixing walkers given as arrays with walkers in the native upstream's packed form,
    and the all-packed group (one join), stage byte for byte what the all-arrays group does;
    so do a non-contiguous amp and a float32 t (converted copies); wrong lengths are refused."""
    assert len({(len(h["t"]), len(h["m"])) for h in hosts}) == len(hosts)   # ragged
    ref_pin, ref_args = _staged(hosts)
    assert ref_pin.any()
    alive = []
    mixed = [_packed(h, alive) if i % 2 else h for i, h in enumerate(hosts)]
    assert any("_src" in h for h in mixed) and any("_src" not in h for h in mixed)
    for walkers in (mixed, [_packed(h, alive) for h in hosts]):
        pin, args = _staged(walkers)
        np.testing.assert_array_equal(pin, ref_pin)
        assert args == ref_args
    # converted inputs: amp as a transposed view, t in float32 (the reference takes its values)
    t32 = hosts[1]["t"].astype(np.float32)
    odd = dict(hosts[1], t=t32, amp=np.asfortranarray(hosts[1]["amp"]))
    assert not odd["amp"].flags.c_contiguous
    plain = dict(hosts[1], t=t32.astype(np.float64))
    pin, args = _staged([hosts[0], odd])
    pin2, args2 = _staged([hosts[0], plain])
    np.testing.assert_array_equal(pin, pin2)
    assert args == args2
    with pytest.raises(ValueError):
        _staged([hosts[0], dict(hosts[1], phi_r=hosts[1]["phi_r"][:-1])])
    with pytest.raises(ValueError):
        _staged([dict(hosts[0], m=hosts[0]["m"][:-1]), hosts[1]])


def test_stage_batch_rejects_bad_input():
    lib = _lib.load()
    tmpl = _lib.ModesumArgs()
    args = (_lib.ModesumArgs * 1)()
    total = ctypes.c_size_t(0)
    src = np.zeros((1, 10), dtype=np.uint64)
    shape = np.array([[5, 2]], dtype=np.int32)
    scale = np.zeros((1, 2))
    pin = np.zeros(1 << 16, dtype=np.uint8)
    assert lib.efd_stage_batch(pin.ctypes.data, pin.nbytes, 0, 1, src.ctypes.data,
                               shape.ctypes.data, scale.ctypes.data, ctypes.byref(tmpl), args,
                               ctypes.byref(total)) == _lib.EFD_ERR_ARG      # NULL source
    shape[0] = (1, 2)
    assert lib.efd_stage_batch(pin.ctypes.data, pin.nbytes, 0, 1, src.ctypes.data,
                               shape.ctypes.data, scale.ctypes.data, ctypes.byref(tmpl), args,
                               ctypes.byref(total)) == _lib.EFD_ERR_ARG      # nt < 2
    assert lib.efd_stage_batch(pin.ctypes.data, pin.nbytes, 0, 0, src.ctypes.data,
                               shape.ctypes.data, scale.ctypes.data, ctypes.byref(tmpl), args,
                               ctypes.byref(total)) == _lib.EFD_ERR_ARG      # empty batch
