"""Build libemrifd.so in-tree (no JIT cache, so the .so travels with the repo snapshot). Every
source is compiled to an object under build/, all of them at once, and one link step follows:

  csrc/emrifd_cpu.cpp, emrifd_reduce_cpu.cpp -> g++ -O3 -march=x86-64-v4 -fopenmp
                         -ffp-contract=off each (the host twins, efd_*_cpu: the mode sum's, the
                         reductions' and the noise draws'; AVX-512 is on both this container's
                         Sapphire Rapids and the GPU box's EPYC 9575F)
  csrc/emrifd_host.cpp -> g++ -O3 -fopenmp -ffp-contract=off: the host upstream stand-ins
  (trajectory, p0 solve) in C++, the walker batches' staging and the PSD table of the
  noise-weighted mode selection (its NaN and sign guards need a unit built without -ffast-math).
  The integrator and the root solve are csrc/emrifd_rk45.h and the table's evaluation is
  csrc/emrifd_psd.h: one text each for this unit and the device (emrifd_traj.hip;
  emrifd_modes_device.inc), both built without contraction; emrifd_modes.cpp (-ffast-math) must
  not include emrifd_rk45.h and does not define EFD_HD for emrifd_psd.h
  csrc/emrifd_modes.cpp -> g++ -O3 -ffast-math -fopenmp (libmvec; knots over threads for one-at-a-time
                          calls): amplitudes, mode selection
  csrc/emrifd.hip, emrifd_prepare.hip, emrifd_window.hip, emrifd_reduce.hip (HIP_UNITS: the mode
                         sum, its preparation, the window path, the channel split and reductions)
                         and emrifd_traj.hip (UPSTREAM_HIP_UNITS: the device trajectories and p0
                         solve, upstream of that chain) and emrifd_noise.hip (NOISE_HIP_UNITS:
                         the noise draws and their overlaps; csrc/emrifd_noise.h is shared with
                         emrifd_reduce_cpu.cpp)
                         -> hipcc --offload-arch=gfx950 -c each; all share csrc/emrifd_common.h,
                         the first two also csrc/emrifd_layout.h (no relocatable device code);
                         emrifd_prepare.hip includes csrc/emrifd_modes_device.inc (amplitudes and
                         mode selection on the device); emrifd_traj.hip includes
                         csrc/emrifd_rk45.h and csrc/traj_costab.inc (the host's cosine table)
  link                -> hipcc -shared over the ten objects, with libgomp and libmvec
"""

import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SRC = os.path.join(CSRC, "emrifd.hip")
# the HIP translation units, the mode sum (SRC) first, then its preparation: the two longest
HIP_UNITS = [SRC, os.path.join(CSRC, "emrifd_prepare.hip"), os.path.join(CSRC, "emrifd_window.hip"),
             os.path.join(CSRC, "emrifd_reduce.hip")]
# the HIP units upstream of that chain (the same flags; they share emrifd_common.h only)
UPSTREAM_HIP_UNITS = [os.path.join(CSRC, "emrifd_traj.hip")]
# the noise realisations' unit (the same flags; six HIP units in all)
NOISE_HIP_UNITS = [os.path.join(CSRC, "emrifd_noise.hip")]
ALL_HIP_UNITS = HIP_UNITS + UPSTREAM_HIP_UNITS + NOISE_HIP_UNITS
CPU_SRC = os.path.join(CSRC, "emrifd_cpu.cpp")
REDUCE_CPU_SRC = os.path.join(CSRC, "emrifd_reduce_cpu.cpp")
HOST_SRC = os.path.join(CSRC, "emrifd_host.cpp")
MODES_SRC = os.path.join(CSRC, "emrifd_modes.cpp")
OUT = os.path.join(HERE, "libemrifd.so")
OBJDIR = os.path.join(HERE, "build")
ARCH = os.environ.get("EFD_OFFLOAD_ARCH", "gfx950")
CPU_ARCH = os.environ.get("EFD_CPU_ARCH", "x86-64-v4")
LINK_LIBS = ["-lgomp", "-lmvec"]


def obj_path(src):
    """The object under OBJDIR that src compiles to."""
    return os.path.join(OBJDIR, os.path.splitext(os.path.basename(src))[0] + ".o")


HOST_OBJS = [obj_path(s) for s in (CPU_SRC, REDUCE_CPU_SRC, HOST_SRC, MODES_SRC)]


def hip_compile_cmd(src, obj, flags=()):
    """One HIP unit to an object (also how an experiment compiles its variant of a unit)."""
    return ["hipcc", f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", *flags, "-c", src,
            "-o", obj]


def link_cmd(objs, out):
    return ["hipcc", f"--offload-arch={ARCH}", "-fPIC", "-shared", "-o", out, *objs, *LINK_LIBS]


def _inputs():
    """Every file the library is compiled from: all of csrc/ (a new source or header needs no
    entry here) and the public header."""
    hdr = os.path.join(os.path.dirname(HERE), "include", "emrifd.h")
    return [p for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p)] + [hdr]


def source_id():
    """16 hex digits of the SHA-256 over the library's sources (name and contents, sorted): the
    build id compiled into libemrifd.so (efd_build_id)."""
    import hashlib
    h = hashlib.sha256()
    for p in sorted(_inputs()):
        if os.path.exists(p):
            h.update(os.path.basename(p).encode() + b"\0")
            h.update(open(p, "rb").read())
    return h.hexdigest()[:16]


def built_id(path=OUT):
    """The build id tagged into an existing library file (read from its bytes, not loaded), or
    None."""
    try:
        data = open(path, "rb").read()
    except OSError:
        return None
    i = data.find(b"EFD_BUILD_ID=")
    if i < 0:
        return None
    j = data.find(b"\0", i)
    return data[i + 13:j].decode(errors="replace")


def build(force=False, verbose=False, extra=()):
    """Compile libemrifd.so unless the in-tree one was built from exactly these sources (its
    tagged build id equals source_id(): content, not file times, so a library that travelled
    with the tree is reused only when it matches; anything else is rebuilt)."""
    sid = source_id()
    if not force and not extra and built_id() == sid:
        return OUT
    os.makedirs(OBJDIR, exist_ok=True)
    gxx = ["g++", "-O3", f"-march={CPU_ARCH}", "-fPIC", "-std=c++17", "-fopenmp"]
    bid = [f'-DEFD_BUILD_ID="{sid}"'] if not extra else []
    # the longest compile (the mode sum) first; ten compilers at once, one per source
    cmds = [hip_compile_cmd(s, obj_path(s), (*bid, *extra)) for s in ALL_HIP_UNITS]
    cmds += [[*gxx, "-ffp-contract=off", "-c", s, "-o", obj_path(s)]
             for s in (CPU_SRC, REDUCE_CPU_SRC, HOST_SRC)]
    cmds += [[*gxx, "-ffast-math", "-c", MODES_SRC, "-o", obj_path(MODES_SRC)]]
    procs = []
    for cmd in cmds:
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append(subprocess.Popen(cmd))
    failed = [cmd for cmd, p in zip(cmds, procs) if p.wait() != 0]   # (waits for every one)
    if failed:
        raise subprocess.CalledProcessError(1, failed[0])
    link = link_cmd(HOST_OBJS + [obj_path(s) for s in ALL_HIP_UNITS], OUT + ".tmp")
    if verbose:
        print(" ".join(link), flush=True)
    subprocess.run(link, check=True)
    os.replace(OUT + ".tmp", OUT)
    return OUT


if __name__ == "__main__":
    print(build(force=True, verbose=True))
