"""The ledger of the networks' stride-1 3x3x3 convolutions (tests/conv_layers.py) against the library's routing, on the host:
every pass (forward with the variant the layer launches, data gradient, weight gradient) of every row, at B = 1 and 2, names a
GPU test case that runs that pass in the same kernel family (modet_conv3d_kernel_family_v) and, where that is the exact-f32
family 0, in the same plan class.  A workload layer without such a case fails here."""
import pytest

from tests import conv_layers as cl


@pytest.fixture(scope="module")
def L():
    from smilecode_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def pool():
    return cl.stand_in_cases()


def test_plan_classes_at_their_thresholds():
    """the documented thresholds, once: each side of every one"""
    assert [cl.fwd_cfg(n, 8, 8) for n in (59999, 60000)] == [8, 0]
    assert [cl.fwd_cfg(n, 8, 64) for n in (7999, 8000, 59999, 60000)] == [6, 7, 7, 2]
    assert [cl.fwd_cfg(n, 8, 32) for n in (59999, 60000, 599999, 600000)] == [6, 5, 5, 1]
    assert [cl.fwd_cfg(60000, ci, 16) for ci in (4, 5)] == [4, 0] and [cl.fwd_cfg(60000, 8, co) for co in (16, 17, 32, 33, 64, 65)] == [0, 5, 5, 2, 2, 3]
    assert cl.fwd_class(60000, 43, 8) == (0, False, True, 2) and cl.fwd_class(60000, 8, 3) == (0, True, False, 4)
    assert cl.fwd_class(60000, 3, 16) == (4, False, False, 1) and cl.fwd_class(59999, 43, 8) == (8, False, True, 1)
    assert [cl.wgrad_class(999999, ci, 32) for ci in (3, 6, 12, 24, 43, 48)] == [(4, 2), (8, 2), (4, 2), (8, 2), (16, 2), (16, 2)]
    assert cl.wgrad_class(1000000, 3, 16) == (4, 4) and cl.wgrad_class(1000000, 16, 16) == (16, 2)


@pytest.mark.parametrize("network", list(cl.NETWORKS))
@pytest.mark.parametrize("B", [1, 2])
def test_every_pass_of_every_layer_has_a_stand_in_in_its_family_and_class(L, pool, network, B):
    rows = cl.layers(network, B)
    assert rows and all(len(r) == 9 for r in rows)
    for row in rows:
        got = cl.stand_ins(L, row)                            # KeyError: no stand-in for a pass of this layer
        assert set(got) == ({"fwd", "wgrad"} if row[5] == 1 else {"fwd", "dgrad", "wgrad"}), row
        for p, (sig, key) in got.items():
            assert key in pool, (row, p, key)
            assert p in pool[key][5], "%s: %s does not check the %s pass" % (row, key, p)
            assert sig in cl.case_signatures(L, pool[key]), "%s %s: %s runs %s" % (row, sig, key, sorted(
                cl.case_signatures(L, pool[key]), key=str))


def test_the_table_names_no_case_it_does_not_need(L, pool):
    used = set()
    for network in cl.NETWORKS:
        for B in (1, 2):
            for row in cl.layers(network, B):
                used |= {sig for sig, _ in cl.stand_ins(L, row).values()}
    assert used == set(cl.STAND_IN)


def test_the_issues_table_of_families(L):
    """the launches the exact-f32 tests were written for: a two-pair PR++ / PCNet step at full resolution"""
    fam = lambda B, ci, co: tuple(L.modet_conv3d_kernel_family_v(B, 160, 192, 160, ci, co, p, 0) for p in (0, 1, 2))      # noqa: E731
    assert [fam(1, ci, co) for ci, co in ((43, 43), (59, 59), (43, 8), (8, 3), (16, 3), (59, 16), (3, 16), (24, 16))] == [
        (5, 5, 0), (5, 5, 0), (5, 5, 4), (5, 5, 4), (5, 5, 4), (5, 5, 4), (5, 5, 0), (5, 5, 4)]
    assert [fam(2, ci, co) for ci, co in ((43, 43), (59, 59), (43, 8), (8, 3), (16, 3), (59, 16), (3, 16), (24, 16))] == [
        (0, 0, 0), (0, 0, 0), (0, 0, 4), (0, 0, 4), (0, 0, 4), (0, 0, 0), (0, 0, 0), (0, 1, 4)]
