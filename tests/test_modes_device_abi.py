"""C ABI of the device-side amplitudes and mode selection (efd_modes_select_batch,
efd_modes_workspace_bytes): host-only checks, no device call is made (runs without a GPU)."""

import ctypes
import os
import subprocess

import pytest

from emri_frequencydomainwaveforms_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_and_exported():
    lib = _lib.load()
    for name in ("efd_modes_select_batch", "efd_modes_workspace_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.efd_version() == 100


def test_workspace_query_is_host_only():
    lib = _lib.load()
    assert lib.efd_modes_workspace_bytes(95, 3843) > 0
    assert lib.efd_modes_workspace_bytes(1, 1) > 0
    assert lib.efd_modes_workspace_bytes(95, 4096) > 0
    assert lib.efd_modes_workspace_bytes(0, 3843) == 0
    assert lib.efd_modes_workspace_bytes(-1, 3843) == 0
    assert lib.efd_modes_workspace_bytes(95, 0) == 0
    assert lib.efd_modes_workspace_bytes(95, 4097) == 0


def _walker(fake, nt=10):
    w = _lib.ModesWalker()
    for f in ("p", "e", "ylm_p", "ylm_m", "keep", "nkeep", "status", "amp", "m_out", "n_out",
              "ylm_p_out", "ylm_m_out", "workspace"):
        setattr(w, f, fake)
    w.nt, w.eps, w.include_minus_m, w.amp_cap, w.workspace_bytes = nt, 1e-2, 1, 1 << 20, 1 << 30
    return w


def test_argument_errors_are_host_side():
    """NULL arguments, count = 0 and count = 17 return EFD_ERR_ARG with the call's name in
    efd_last_error before anything touches the device (the pointers are never dereferenced)."""
    lib = _lib.load()
    fake = 1 << 12
    buf = ctypes.create_string_buffer(256)
    tab = _lib.ModesTable(fake, fake, fake, fake, fake, 3843)
    ws = (_lib.ModesWalker * 17)(*[_walker(fake + 4096 * i) for i in range(17)])

    def err(*args):
        rc = lib.efd_modes_select_batch(*args)
        lib.efd_last_error(buf, 256)
        return rc, buf.value

    rc, msg = err(None, ws, 1, None)
    assert rc == -1 and msg.startswith(b"efd_modes_select_batch: NULL argument")
    rc, msg = err(ctypes.byref(tab), None, 1, None)
    assert rc == -1 and msg.startswith(b"efd_modes_select_batch: NULL argument")
    for count in (0, 17, -3):
        rc, msg = err(ctypes.byref(tab), ws, count, None)
        assert rc == -1 and msg.startswith(b"efd_modes_select_batch: count out of range")
    # the mode table: a NULL array, nmodes outside [1, 4096]
    bad = _lib.ModesTable(fake, None, fake, fake, fake, 3843)
    rc, msg = err(ctypes.byref(bad), ws, 1, None)
    assert rc == -1 and b"efd_modes_select_batch: NULL mode table" in msg
    for nm in (0, 4097):
        bad = _lib.ModesTable(fake, fake, fake, fake, fake, nm)
        rc, msg = err(ctypes.byref(bad), ws, 1, None)
        assert rc == -1 and b"efd_modes_select_batch: nmodes out of range" in msg
    # a walker: a NULL pointer, nt, eps, the workspace
    for field in ("p", "ylm_m", "keep", "status", "ylm_m_out", "workspace"):
        w = (_lib.ModesWalker * 1)(_walker(fake))
        setattr(w[0], field, None)
        rc, msg = err(ctypes.byref(tab), w, 1, None)
        assert rc == -1 and b"efd_modes_select_batch: NULL walker pointer" in msg, field
    for field, val, text in (("nt", 0, b"nt out of range"), ("nt", 1025, b"nt out of range"),
                             ("eps", -1e-3, b"eps out of range"),
                             ("eps", float("nan"), b"eps out of range"),
                             ("amp_cap", -1, b"amp_cap")):
        w = (_lib.ModesWalker * 1)(_walker(fake))
        setattr(w[0], field, val)
        rc, msg = err(ctypes.byref(tab), w, 1, None)
        assert rc == -1 and text in msg, field
    w = (_lib.ModesWalker * 1)(_walker(fake))
    w[0].workspace_bytes = lib.efd_modes_workspace_bytes(10, 3843) - 1
    rc, msg = err(ctypes.byref(tab), w, 1, None)
    assert rc == -3 and b"efd_modes_select_batch: workspace too small" in msg
    # two walkers on one workspace
    w = (_lib.ModesWalker * 2)(_walker(fake), _walker(fake))
    rc, msg = err(ctypes.byref(tab), w, 2, None)
    assert rc == -1 and b"per walker" in msg


@pytest.mark.parametrize("cname,pycls", [("efd_modes_table", "ModesTable"),
                                         ("efd_modes_walker", "ModesWalker")])
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
