"""GPU: rxg_flow_trains_dev on the edge sets of tests/flowtrain_edge_cases.py -- a left-out count
in slice 64 and in slice 1 024 (the second wave's share of the two sums, and the loop's second
trip), three sort passes over four tiles with every digit live (and the same burst in two, so the
sorted list ends in the other buffer), a digit that lives in one wave-round of a tile, train
starts on the last and first lane of a wave, a round and a tile, a tile without a start between
two that have some, 255 / 256 / 257 trains and a HEAD whose cur_seq index needs three bytes, and
the order of the tests in the record decode -- against the model tests/flowtrain_ref.py, never the
kernels' own output or the host function (tests/test_flowtrain_edge_cases_host.py pins that one
to the model on the same sets and holds the sets to their claims).  Each set is one parameter and
runs in every layout (REC16 through a stride, the others through off64) on the default grid and
with max_blocks 1 and 2: each run's bytes equal the model's, and the runs equal each other.  Same
discipline as test_gpu_flowtrain.py: outputs pre-filled with 0xA5 and compared whole, eight guard
entries behind `order` and `trains` and the words around `count` included; no tolerance anywhere."""
import pytest

import flowtrain_edge_cases as ec
import rxg
from test_gpu_flowtrain import Batch

pytestmark = pytest.mark.gpu

EDGE = ec.edge_cases()


@pytest.fixture(scope="module")
def capped():
    engs = [rxg.Engine(device=0, max_blocks=1), rxg.Engine(device=0, max_blocks=2)]
    yield engs
    for e in engs:
        e.close()


@pytest.mark.parametrize("case", EDGE, ids=lambda c: c.name)
def test_edge_sets_in_every_layout_on_three_grids(engine, capped, case):
    grids = [(engine, "default grid"), (capped[0], "max_blocks 1"), (capped[1], "max_blocks 2")]
    for kind in ec.kinds(case):
        stride = kind == rxg.REC16
        b = Batch.of(engine, case, kind, strided=stride)
        try:
            assert b.wcount.tolist()[:2] == [b.S, b.T] and b.S > 1 and b.T > 0
            for cap_trains in [None] + case.claims.get("cap_trains", []):
                got = [b.run(eng, what=f"{case.name}, records of {kind}, {grid}, cap_trains {cap_trains}",
                             cap_trains=cap_trains, use_stride=stride) for eng, grid in grids]
                assert got[0] == got[1] == got[2], (case.name, kind, cap_trains)
        finally:
            b.close()
