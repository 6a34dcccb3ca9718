"""What compare_bvh8_canonical - the tree comparison of the device-build parity tests
(test_gpu_lbvh_parity.py) - notices, tried without a GPU by ark_ddgi_debug_bvh8_compare_selftest
on test_lbvh.py's 20,000-triangle soup dealt to three classes, and on the sun's light build of
it: a twin whose nodes and rows are renumbered within each level, as the device's atomics do,
compares clean, and each of six mutations of the twin is reported."""
import pytest

from arkoserenderer_amd import ddgi as D

from test_lbvh import soup

SUNS = {"world": None, "sun": (0.3, -1.0, -0.4)}
MUTATIONS = ("plane_looser", "grid_coarser", "children_exchanged", "leaf_members_exchanged", "records_exchanged", "perm_altered")


@pytest.fixture(scope="module", params=list(SUNS))
def selftest(request):
    rc, r = D.bvh8_compare_selftest(soup(), SUNS[request.param], seed=20260)
    print(request.param, rc, r)
    return rc, r


def test_renumbered_twin_compares_clean(selftest):
    rc, r = selftest
    assert r["nodes"] > 1000 and r["renumbered"] > r["nodes"] // 2, r  # the twin really is another numbering
    assert r["twin_differences"] == 0 and r["pairs"] == r["nodes"], r
    assert r["twin_violations"] == 0, r  # ... and a valid tree


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_mutation_is_reported(selftest, mutation):
    rc, r = selftest
    assert r[mutation] > 0, r


def test_full_check_passes_looser_boxes(selftest):
    """The gap the canonical comparison closes: a plane one quantum too loose and a grid one
    exponent too coarse are valid trees, so check_bvh8_full - all that looked at a device
    build's boxes before - reports no violation for either; the comparison reports both
    (test_mutation_is_reported)."""
    rc, r = selftest
    assert r["full_check_plane_looser"] == 0 and r["full_check_grid_coarser"] == 0, r
    assert r["plane_looser"] > 0 and r["grid_coarser"] > 0, r


def test_selftest_return_code(selftest):
    rc, r = selftest
    assert rc == 0, r
