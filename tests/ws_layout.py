"""Python mirror of the mode sum's workspace layout (csrc/emrifd_layout.h): make_layout, the
288-B interval record `Item` and the 64-B `Header`, for tests that read a prepared workspace
(ModeSumEngine._ws, a torch byte tensor) directly.

The constants are restated as literals, each beside its header name; tests/test_ws_layout.py holds
`total` of the unpaired mirror to efd_modesum_workspace_bytes exactly, so the mirror cannot drift
from the header unnoticed, and tests/test_gpu_records.py cross-checks the offsets against a
workspace the device wrote.
"""

from collections import namedtuple

import numpy as np

TILE = 256                  # TILE (emrifd_constants.h)
EFD_BPL = 3                 # EFD_BPL / BPL (emrifd_constants.h)
TILE_LANES = TILE * EFD_BPL  # TILE_LANES
MAXRUNS = 8                 # MAXRUNS (emrifd_constants.h)
MAX_NT = 1024               # MAX_NT (emrifd_constants.h)
MAX_K = 8192                # MAX_K (emrifd_constants.h)
SEG1_NT = 1024              # SEG1_NT
SEG1_MAX_K = SEG1_NT // (2 * MAXRUNS)   # SEG1_MAX_K = 64
KEYCAP = 2048               # KEYCAP
SPLIT_ITEM_CAP = 8192       # SPLIT_ITEM_CAP
SPLIT_TILE_CAP = 128        # SPLIT_TILE_CAP
HDR_MAGIC = 0x45464448445233    # HDR_MAGIC, "EFDHDR3"

# struct Item, field by field in the header's order
ITEM = np.dtype([
    ("gx", "<f8"), ("ic", "<f8", (4,)), ("tj", "<f8"), ("ph", "<f8", (4,)),
    ("fd", "<f8", (3,)), ("dtj", "<f8"), ("fdd", "<f8", (3,)),
    ("jser", "<i4"), ("fdneg", "<i4"),
    ("b", "<f8", (2, 2, 4)), ("klo", "<i4", (2,)), ("khi", "<i4", (2,))])
assert ITEM.itemsize == 288
# ENV_DEG (env_fit.inc): an envelope record's fd, dtj, fdd slots hold A's ENV_DEG + 1 coefficients
ENV_DEG = 6
ENV_OFFSET = ITEM.fields["fd"][1]
assert (ITEM.fields["dtj"][1] == ENV_OFFSET + 24 and ITEM.fields["fdd"][1] == ENV_OFFSET + 32
        and ITEM.fields["jser"][1] == ENV_OFFSET + 8 * (ENV_DEG + 1))

# struct Header
HEADER = np.dtype([
    ("contributions", "<i8"), ("evaluations", "<i8"), ("runs_overflow", "<i4"),
    ("groups", "<i4"), ("bad_mn", "<i4"), ("bad_tile", "<i4"), ("magic", "<i8"),
    ("lane_lo", "<i4"), ("lane_hi", "<i4"), ("nitems", "<i4"), ("nsplit", "<i4"),
    ("env_evaluations", "<i8")])
assert HEADER.itemsize == 64

_FIELDS = ("header coefA coefT kslope tscratch invcp invdp runs items ranges seglh seginfo nseg "
           "slotlh slotinfo slotcnt slottiles segbase stb0 stb1 gm gn gstart gmem gkeys gamp sctab "
           "tkeys tcnt tperm llpart sitem scnt spart total stbcap ntiles nlanes").split()
Layout = namedtuple("Layout", _FIELDS)


def align256(x):
    return (x + 255) & ~255


def make_layout(nt, K, nf, paired):
    """make_layout of emrifd_layout.h: byte offsets of every workspace buffer, `total`, and the
    lane / tile counts, for N_t knots, K harmonics and nf bins."""
    ni = nt - 1
    nlanes = (nf + 1) // 2 if paired else nf
    ntiles = (nlanes + TILE_LANES - 1) // TILE_LANES
    off = [0]
    o = {}

    def take(name, nbytes):
        o[name] = off[0]
        off[0] = align256(off[0] + nbytes)

    slots = 2 * MAXRUNS * K
    take("header", HEADER.itemsize)
    take("coefA", 8 * ni * 4 * 4 * K)
    take("coefT", 8 * ni * 4 * 8)
    take("kslope", 8 * nt * 2)
    take("tscratch", 8 * nt * 16)
    take("invcp", 8 * nt * K)
    take("invdp", 8 * nt * K)
    take("runs", 4 * 4 * MAXRUNS * K)
    take("items", ITEM.itemsize * ni * K)
    take("ranges", 16 * ni * K)          # int4
    take("seglh", 8 * slots)             # int2
    take("seginfo", 16 * slots)          # int4
    take("nseg", 4)
    take("slotlh", 8 * slots)
    take("slotinfo", 16 * slots)
    take("slotcnt", 4 * ((slots + 255) // 256))
    take("slottiles", 4 * ((slots + 255) // 256))
    take("segbase", 4 * slots)
    stbcap = 64 * ntiles + 4 * slots
    take("stb0", 4 * stbcap)
    take("stb1", 4 * stbcap)
    take("gm", 4 * K)
    take("gn", 4 * K)
    take("gstart", 4 * (K + 1))
    take("gmem", 4 * K)
    take("gkeys", 8 * MAX_K)
    take("gamp", 8 * nt * 4 * K)
    take("sctab", 8 * 2 * 512)
    take("tkeys", 4 * ntiles * KEYCAP)
    take("tcnt", 4 * ntiles)
    take("tperm", 4 * ntiles)
    take("llpart", 8 * ntiles)
    plan = K <= SEG1_MAX_K
    take("sitem", 16 * SPLIT_ITEM_CAP if plan else 0)
    take("scnt", 4 * SPLIT_TILE_CAP if plan else 0)
    take("spart", 8 * 4 * SPLIT_TILE_CAP * TILE_LANES if plan else 0)
    return Layout(total=off[0], stbcap=stbcap, ntiles=ntiles, nlanes=nlanes, **o)


def read_workspace(ws_bytes, nt, K, nf, paired):
    """The preparation's output in a workspace downloaded as a uint8 numpy array: dict of header
    (HEADER scalar), coefT [ni][4][8], coefA [ni][4][4K], gm, gn [G], gstart [G + 1] and items
    [G][ni] (ITEM records of group g, interval j at [g][j])."""
    L = make_layout(nt, K, nf, paired)
    ni = nt - 1
    ws = np.ascontiguousarray(ws_bytes, dtype=np.uint8)
    assert ws.size >= L.total

    def at(off, dtype, count):
        dt = np.dtype(dtype)
        return ws[off:off + dt.itemsize * count].view(dt).copy()

    hdr = at(L.header, HEADER, 1)[0]
    G = int(hdr["groups"])
    assert 0 <= G <= K
    return dict(layout=L, header=hdr, groups=G,
                coefT=at(L.coefT, "<f8", ni * 32).reshape(ni, 4, 8),
                coefA=at(L.coefA, "<f8", ni * 16 * K).reshape(ni, 4, 4 * K),
                gm=at(L.gm, "<i4", G), gn=at(L.gn, "<i4", G), gstart=at(L.gstart, "<i4", G + 1),
                items=at(L.items, ITEM, G * ni).reshape(G, ni))
