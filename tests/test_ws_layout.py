"""tests/ws_layout.py cannot drift from csrc/emrifd_layout.h unnoticed: the mirror's workspace
size equals efd_modesum_workspace_bytes (make_layout's unpaired `total`, a host-only query) on
shapes that reach every term of the layout."""

import pytest

from emri_frequencydomainwaveforms_amd import _lib
from tests import ws_layout

# (N_t, K, N_f): K on both sides of SEG1_MAX_K (the split plan's buffers), nf = 1, nf around a
# tile of lanes (768) and around a paired tile (1535 .. 1537), the smallest and largest N_t, a
# slot count that is no multiple of 256, the flagship size
SHAPES = [(45, 75, 31559), (34, 1049, 15781), (2, 1, 1), (4, 64, 768), (4, 65, 768),
          (45, 63, 767), (45, 64, 769), (100, 65, 1535), (100, 17, 1536), (100, 3000, 1537),
          (1024, 8192, 3), (1000, 3020, 6311631)]


@pytest.mark.parametrize("nt,K,nf", SHAPES)
def test_mirror_total_equals_workspace_bytes(nt, K, nf):
    lib = _lib.load()
    want = int(lib.efd_modesum_workspace_bytes(nt, K, nf))
    assert want > 0
    L = ws_layout.make_layout(nt, K, nf, 0)
    assert L.total == want
    # the paired layout has fewer lanes and never needs more (the query sizes by the unpaired one)
    P = ws_layout.make_layout(nt, K, nf, 1)
    assert P.total <= L.total and P.nlanes == (nf + 1) // 2 and L.nlanes == nf
    # offsets ascend, 256-B aligned, and the record block holds N_i K records
    names = ws_layout.Layout._fields
    offs = [getattr(L, f) for f in names[:names.index("total")]]
    assert offs[0] == 0 and all(o % 256 == 0 for o in offs)
    assert offs == sorted(offs)
    assert L.ranges - L.items >= ws_layout.ITEM.itemsize * (nt - 1) * K


def test_record_and_header_sizes():
    assert ws_layout.ITEM.itemsize == 288 and ws_layout.HEADER.itemsize == 64
    # the package's own two header numbers (ModeSumEngine._workspace, split_plan)
    assert _lib.HEADER_BYTES == ws_layout.HEADER.itemsize
    assert _lib.HEADER_SPLIT_PLAN == ws_layout.HEADER.fields["nitems"][1]
    assert ws_layout.HEADER.fields["nsplit"][1] == _lib.HEADER_SPLIT_PLAN + 4
    assert ws_layout.ITEM.names == ("gx", "ic", "tj", "ph", "fd", "dtj", "fdd", "jser", "fdneg",
                                    "b", "klo", "khi")
    assert ws_layout.SEG1_MAX_K == 64 and ws_layout.TILE_LANES == 768
