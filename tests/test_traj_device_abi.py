"""C ABI of the device trajectories and p0 solve (efd_traj_batch, efd_traj_p_at_t_batch):
host-only checks, no device call is made (runs without a GPU)."""

import ctypes
import math
import os
import re
import subprocess
from fractions import Fraction

from emri_frequencydomainwaveforms_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "emrifd.h")
COSTAB = os.path.join(ROOT, "emri_frequencydomainwaveforms_amd", "csrc", "traj_costab.inc")
# emrifd_host.cpp's TWO_PI literal (the double nearest 2 pi)
TWO_PI = 6.283185307179586476925286766559005768


def _flat(txt):
    """C text without comments, whitespace runs as one blank."""
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", txt, flags=re.S))


def test_symbols_exist_with_the_headers_signatures():
    lib = _lib.load()
    hdr = _flat(open(HEADER).read())
    for name in ("efd_traj_batch", "efd_traj_p_at_t_batch"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert ("int efd_traj_batch(const efd_traj_source* src , int32_t count, int32_t max_len, "
            "double* knots , int32_t* nt , int32_t* status , void* stream);") in hdr
    assert ("int efd_traj_p_at_t_batch(const efd_traj_source* src , int32_t count, double xtol, "
            "double rtol_root, double* p0 , int32_t* status, void* stream);") in hdr
    assert ("typedef struct efd_traj_source { double M, mu, p0, e0, Phi_phi0, Phi_r0, T, rtol, "
            "atol; } efd_traj_source;") in hdr
    vp, i32, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    assert lib.efd_traj_batch.argtypes == [vp, i32, i32, vp, vp, vp, vp]
    assert lib.efd_traj_p_at_t_batch.argtypes == [vp, i32, dbl, dbl, vp, vp, vp]
    for name, val in (("EFD_TRAJ_MAX_LEN", 1024), ("EFD_TRAJ_OK", 0), ("EFD_TRAJ_BAD_SOURCE", 1),
                      ("EFD_TRAJ_TOO_LONG", 2), ("EFD_TRAJ_STEP_FAILED", 3),
                      ("EFD_TRAJ_STEP_CAP", 4), ("EFD_TRAJ_NO_BRACKET", 5)):
        assert re.search(rf"#define {name} {val}\b", hdr), name
        assert getattr(_lib, name) == val


def test_argument_errors_are_host_side():
    """NULL pointers, count < 1 and a max_len outside 2..1024 return EFD_ERR_ARG with the call's
    name in efd_last_error before any launch (the fake pointers are never dereferenced)."""
    lib = _lib.load()
    fake = 1 << 12
    buf = ctypes.create_string_buffer(256)

    def err(fn, *args):
        rc = fn(*args)
        lib.efd_last_error(buf, 256)
        return rc, buf.value

    good = [fake, 1, 100, fake, fake, fake, None]
    for i in (0, 3, 4, 5):
        a = list(good)
        a[i] = None
        rc, msg = err(lib.efd_traj_batch, *a)
        assert rc == _lib.EFD_ERR_ARG and msg.startswith(b"efd_traj_batch: NULL pointer"), i
    for count in (0, -1):
        rc, msg = err(lib.efd_traj_batch, fake, count, 100, fake, fake, fake, None)
        assert rc == _lib.EFD_ERR_ARG and msg.startswith(b"efd_traj_batch: count < 1")
    for max_len in (1, 0, -5, 1025):
        rc, msg = err(lib.efd_traj_batch, fake, 1, max_len, fake, fake, fake, None)
        assert rc == _lib.EFD_ERR_ARG and msg.startswith(b"efd_traj_batch: max_len"), max_len
    good = [fake, 1, 2e-12, 8.9e-16, fake, fake, None]
    for i in (0, 4, 5):
        a = list(good)
        a[i] = None
        rc, msg = err(lib.efd_traj_p_at_t_batch, *a)
        assert rc == _lib.EFD_ERR_ARG and msg.startswith(b"efd_traj_p_at_t_batch: NULL pointer")
    for count in (0, -7):
        rc, msg = err(lib.efd_traj_p_at_t_batch, fake, count, 2e-12, 8.9e-16, fake, fake, None)
        assert rc == _lib.EFD_ERR_ARG and msg.startswith(b"efd_traj_p_at_t_batch: count < 1")


def _cos_rounded(x):
    """cos of the double x correctly rounded: the Taylor series in exact rationals (|x| < 7, 60
    terms leave a remainder below 1e-60), then one rounding."""
    x = Fraction(x)
    term, total, x2 = Fraction(1), Fraction(1), x * x
    for k in range(1, 61):
        term = -term * x2 / ((2 * k - 1) * (2 * k))
        total += term
    return total.numerator / total.denominator   # int / int: correctly rounded


def test_cosine_table_is_the_hosts_bit_for_bit():
    """The committed table's 64 hex floats are the doubles emrifd_host.cpp's CosTable holds:
    cos of the double TWO_PI * i / 64, by the C library the host unit calls (math.cos) and, so
    that a compile-time evaluation of the same expression gives them too, correctly rounded."""
    txt = re.sub(r"//.*", "", open(COSTAB).read())
    vals = [float.fromhex(v) for v in re.findall(r"-?0x[0-9a-fA-F.]+p[-+]?\d+", txt)]
    assert len(vals) == 64
    for i, v in enumerate(vals):
        arg = TWO_PI * i / 64
        assert v.hex() == math.cos(arg).hex(), i
        assert v.hex() == _cos_rounded(arg).hex(), i


def test_struct_layout_matches_c(tmp_path):
    cls = _lib.TrajSource
    fields = [f for f, _ in cls._fields_]
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "emrifd.h"', "int main(void){",
            'printf("%zu\\n", sizeof(efd_traj_source));']
    prog += [f'printf("%zu\\n", offsetof(efd_traj_source, {f}));' for f in fields]
    prog += ["return 0;}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(cls) == 72
    for f, off in zip(fields, out[1:]):
        assert getattr(cls, f).offset == off, f
