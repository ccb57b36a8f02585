"""C ABI: libemrifd.so loads, exports every function include/emrifd.h declares, and the ctypes
mirror of efd_modesum_args has the C layout. No compute calls (runs without a GPU)."""

import ctypes
import os
import re
import subprocess

import pytest

from emri_frequencydomainwaveforms_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "emrifd.h")


def declared_functions():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^\w[\w\s\*]*?\b(efd_\w+)\s*\(", txt, flags=re.M)))


def test_header_and_python_list_agree():
    assert declared_functions() == sorted(_lib.EXPORTED_SYMBOLS)


def test_library_exports_every_symbol():
    if not os.path.exists(_lib.LIB_PATH):
        from emri_frequencydomainwaveforms_amd import _build
        _build.build()
    lib = _lib.load()
    for name in declared_functions():
        assert hasattr(lib, name), name
    assert lib.efd_version() == 100
    # the library that loads was compiled from exactly these sources (a library that travelled
    # with the tree is reused only when its tagged build id matches, _build.build)
    from emri_frequencydomainwaveforms_amd import _build
    assert lib.efd_build_id().decode() == _build.source_id() == _build.built_id()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True, check=True).stdout
    for name in declared_functions():
        assert re.search(rf"\bT {name}$", nm, flags=re.M), name
    # and nothing undeclared: the shipped build exports exactly the header's efd_* functions
    # (efd_exp_* diagnostics exist only in -DEFD_EXP experiment builds)
    exported = sorted(set(re.findall(r"\bT (efd_\w+)$", nm, flags=re.M)))
    assert exported == declared_functions()


def test_build_inputs_cover_every_source_file():
    """Every regular file in csrc/ (and the public header) is in _build._inputs(), so it counts
    in source_id(): a source nobody listed cannot leave a stale libemrifd.so in use. The HIP
    units the build compiles are among them."""
    from emri_frequencydomainwaveforms_amd import _build
    inputs = {os.path.realpath(p) for p in _build._inputs()}
    files = [os.path.join(_build.CSRC, f) for f in os.listdir(_build.CSRC)]
    files = [p for p in files if os.path.isfile(p)]
    assert len(files) >= 13   # 4 HIP units, their 3 headers, 3 host sources, 3 tables
    for p in files:
        assert os.path.realpath(p) in inputs, p
    assert os.path.realpath(HEADER) in inputs
    assert len(_build.HIP_UNITS) == 4 and _build.HIP_UNITS[0] == _build.SRC
    for p in _build.HIP_UNITS:
        assert os.path.isfile(p) and os.path.realpath(p) in inputs, p
        assert os.path.dirname(_build.obj_path(p)) == _build.OBJDIR


def test_last_error_reports_every_unit():
    """efd_last_error holds one string for the library: an argument error raised in the
    preparation unit, the window unit or the reduction unit reads back as the mode sum's do (no
    device call is made)."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    assert lib.efd_upload(None, None, 8, None) == -1              # emrifd.hip
    lib.efd_last_error(buf, 256)
    assert b"efd_upload: NULL pointer" in buf.value
    assert lib.efd_spline_build(None, 0, None, 0, None, None) == -1       # emrifd_prepare.hip
    lib.efd_last_error(buf, 256)
    assert b"efd_spline_build: bad arguments" in buf.value
    assert lib.efd_modesum_prepare_batch(None, None, None, 0, None) == -1
    lib.efd_last_error(buf, 256)
    assert b"efd_modesum_prepare_batch: NULL argument" in buf.value
    assert lib.efd_hann_stage(None, 0, 0, 0, None, 0, None, None) == -1   # emrifd_window.hip
    lib.efd_last_error(buf, 256)
    assert b"efd_hann_stage: bad arguments" in buf.value
    assert lib.efd_polarizations(None, 0, 0, None, None, None) == -1      # emrifd_reduce.hip
    lib.efd_last_error(buf, 256)
    assert b"efd_polarizations: bad arguments" in buf.value
    assert lib.efd_loglike(None, None, None, 0, 0, None, None, None) == -1
    lib.efd_last_error(buf, 256)
    assert b"efd_loglike: bad arguments" in buf.value


def test_workspace_query_is_host_only():
    lib = _lib.load()
    assert lib.efd_modesum_workspace_bytes(100, 3000, 6311631) > 0
    assert lib.efd_modesum_workspace_bytes(1, 3000, 100) == 0
    assert lib.efd_modesum_workspace_bytes(2000, 3000, 100) == 0
    assert lib.efd_td_workspace_bytes(100, 3000) > 0
    assert lib.efd_td_workspace_bytes(1, 3000) == 0
    assert lib.efd_td_workspace_bytes(100, 0) == 0


@pytest.mark.parametrize("cname,pycls", [("efd_modesum_args", "ModesumArgs"),
                                         ("efd_td_args", "TdArgs")])
def test_struct_layout_matches_c(tmp_path, cname, pycls):
    cls = getattr(_lib, pycls)
    fields = [f for f, _ in cls._fields_]
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "emrifd.h"', "int main(void){",
            f'printf("%zu\\n", sizeof({cname}));']
    prog += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f in fields]
    prog += ["return 0;}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(cls)
    for f, off in zip(fields, out[1:]):
        assert getattr(cls, f).offset == off, f


def test_no_cpu_fallback_without_gpu():
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from emri_frequencydomainwaveforms_amd.summation import require_gpu
    with pytest.raises(_lib.EFDError):
        require_gpu()


def test_header_constants_match_python():
    txt = open(HEADER).read()
    defs = dict(re.findall(r"^#define (EFD_\w+) \(?(-?\d+)\)?", txt, flags=re.M))
    for name, val in defs.items():
        if name in ("EFD_VERSION",):
            continue
        assert hasattr(_lib, name), name
        assert getattr(_lib, name) == int(val), name


def test_argument_errors_are_host_side():
    """Shape errors return EFD_ERR_ARG with a message before anything touches the device, e.g.
    a grid of 2^31 - 1 bins or more (lane indices are 32-bit)."""
    lib = _lib.load()
    fake = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    a = _lib.ModesumArgs()
    for f in ("t", "phi_phi", "phi_r", "f_phi", "f_r", "amp", "m", "n", "ylm_p", "ylm_m", "freq",
              "out"):
        setattr(a, f, fake)
    a.nt, a.K, a.caustic, a.scale_re = 100, 3000, 1, 1.0
    a.grid_symmetric = 1
    buf = ctypes.create_string_buffer(256)
    a.nf = 2 ** 31 - 1
    assert lib.efd_modesum(ctypes.byref(a), fake, ctypes.c_size_t(1 << 40), None) == -1
    lib.efd_last_error(buf, 256)
    assert b"nf out of range" in buf.value
    a.nf = 1000
    a.nt = 1
    assert lib.efd_modesum(ctypes.byref(a), fake, ctypes.c_size_t(1 << 40), None) == -1
    lib.efd_last_error(buf, 256)
    assert b"nt out of range" in buf.value


def test_fused_loglike_argument_errors_are_host_side():
    """efd_modesum_sum_loglike rejects, before any device work: NULL d/w/out, an asymmetric
    grid, accumulate = 1, k0 outside [0, nf), and members that disagree on k0."""
    lib = _lib.load()
    fake = ctypes.c_void_p(16)
    a = _lib.ModesumArgs()
    for f in ("t", "phi_phi", "phi_r", "f_phi", "f_r", "amp", "m", "n", "ylm_p", "ylm_m", "freq"):
        setattr(a, f, fake)
    a.nt, a.K, a.caustic, a.scale_re, a.nf, a.k0 = 100, 30, 1, 1.0, 1001, 500
    a.grid_symmetric = 1
    b = _lib.ModesumArgs.from_buffer_copy(a)
    buf = ctypes.create_string_buffer(256)
    ws = (ctypes.c_void_p * 2)(16, 16)
    nb = (ctypes.c_size_t * 2)(1 << 40, 1 << 40)

    def call(x, y, d=fake, w=fake, out=fake):
        pa = (ctypes.POINTER(_lib.ModesumArgs) * 2)(ctypes.pointer(x), ctypes.pointer(y))
        rc = lib.efd_modesum_sum_loglike(pa, ws, nb, 2, d, w, out, None)
        lib.efd_last_error(buf, 256)
        return rc, buf.value

    assert call(a, b, d=None)[0] == -1 and b"NULL d, w or out" in buf.value
    assert call(a, b, out=None)[0] == -1
    for field, bad, both in (("grid_symmetric", 0, True), ("accumulate", 1, True),
                             ("k0", 1001, True), ("k0", 499, False)):
        c = _lib.ModesumArgs.from_buffer_copy(b)
        setattr(c, field, bad)
        a2 = _lib.ModesumArgs.from_buffer_copy(a)
        if both:   # (members that disagree fail the batch's agreement check first)
            setattr(a2, field, bad)
        rc, msg = call(a2, c)
        assert rc == -1 and b"fused likelihood needs" in msg, (field, msg)


def test_tile_constants_and_ordering_argument_errors_are_host_side():
    """efd_loglike_tile_count / _tile_constants, efd_modesum_sum_loglike_ex, efd_download and
    efd_stream_order validate their arguments before any HIP call."""
    lib = _lib.load()
    fake = ctypes.c_void_p(16)
    buf = ctypes.create_string_buffer(256)
    assert lib.efd_loglike_tile_count(0) == 0
    assert lib.efd_loglike_tile_count(6311631) == 4110   # config 4: 3,155,816 lane pairs / 768
    assert lib.efd_loglike_tile_count(1001) >= 1
    assert lib.efd_loglike_tile_constants(None, fake, 1001, 500, fake, None) == -1
    lib.efd_last_error(buf, 256)
    assert b"NULL d, w or tile_const" in buf.value
    assert lib.efd_loglike_tile_constants(fake, fake, 1001, 1001, fake, None) == -1
    lib.efd_last_error(buf, 256)
    assert b"0 <= k0 < nf" in buf.value
    pa = (ctypes.POINTER(_lib.ModesumArgs) * 1)()
    ws = (ctypes.c_void_p * 1)(16)
    nb = (ctypes.c_size_t * 1)(1 << 40)
    assert lib.efd_modesum_sum_loglike_ex(pa, ws, nb, 1, fake, fake, fake, None, None) == -1
    lib.efd_last_error(buf, 256)
    assert b"NULL d, w or out" in buf.value
    assert lib.efd_download(None, fake, 8, None) == -1
    assert lib.efd_download(None, None, 0, None) == 0          # nothing to copy
    assert lib.efd_stream_order(None, None, 0) == 0             # nothing to order
    assert lib.efd_stream_order(None, None, 2) == -1
    lib.efd_last_error(buf, 256)
    assert b"efd_stream_order" in buf.value
