"""CPU checks of the solver knobs (csrc/gn/knobs.h: one table row per knob,
m3s_set_knob): which names each build of the library knows, that a set returns
the value before it, that the environment is read, and that a knob set through
the table reaches the host planner. No GPU needed: the libraries load here as
in tests/test_abi.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PRODUCT = ("plan_cache", "dense_tail_min", "track_persistent", "prologue")
TEST_ONLY = ("dense", "cols", "df", "tail_cyc", "tail_mfma", "border_split", "debug_drop_item", "gather_lds",
             "tail_pair", "tail_warm", "gcomb", "gcomb_wg", "gcomb_min_nc")
UNKNOWN = -(1 << 30)


@pytest.fixture(scope="module")
def be():
    import mast3r_slam_backends as be

    return be


@pytest.mark.parametrize("name", PRODUCT)
def test_product_knob_round_trips(be, name):
    old = be.set_knob(name, 7)
    try:
        assert be.set_knob(name, 9) == 7  # the value before this set
        assert be.set_knob(name, 9) == 9  # also when nothing changes
    finally:
        assert be.set_knob(name, old) == 9
    assert be.set_knob(name, old) == old  # restored


def test_unknown_name_raises(be):
    with pytest.raises(RuntimeError, match="unknown knob"):
        be.set_knob("no_such_knob", 1)
    assert be._lib.m3s_set_knob(b"no_such_knob", 1) == UNKNOWN
    assert be._lib.m3s_set_knob(b"", 1) == UNKNOWN


@pytest.mark.parametrize("name", TEST_ONLY)
def test_test_only_knob_lives_in_the_test_library_only(be, name):
    assert be._lib.m3s_set_knob(name.encode(), 1) == UNKNOWN
    with pytest.raises(RuntimeError, match="unknown knob"):
        be.set_knob(name, 1)
    lib = be.load_test_library()
    old = lib.m3s_set_knob(name.encode(), 3)
    assert old != UNKNOWN
    assert lib.m3s_set_knob(name.encode(), old) == 3


def test_test_library_knows_the_product_knobs(be):
    lib = be.load_test_library()
    for name in PRODUCT:
        old = lib.m3s_set_knob(name.encode(), 5)
        assert old != UNKNOWN
        assert lib.m3s_set_knob(name.encode(), old) == 5


def test_environment_is_read_at_first_use():
    code = ("import mast3r_slam_backends as be\n"
            "assert be.set_knob('dense_tail_min', 5) == 0\n"
            "assert be.set_knob('dense_tail_min', 6) == 5\n"
            "assert be.set_knob('plan_cache', 1) == 1\n")  # no variable set: the default
    env = dict(os.environ, M3S_DENSE_TAIL_MIN="0",
               PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "mast3r-slam-ysh_amd"), os.environ.get("PYTHONPATH", "")]))
    env.pop("M3S_PLAN_CACHE", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_dense_tail_min_reaches_the_planner(be, knobs):
    # the graph of test_sparse_plan.py's dense-tail case (128, 6, 8, 8)
    from mast3r_slam_amd import synthetic

    N = 128
    g = synthetic.make_graph(N, 2, 2, seed=6, edge_range=(0, 0), kf_ids=np.arange(N) * 3 + 5)
    ii, jj = g.ii.numpy(), g.jj.numpy()
    u = np.unique(np.concatenate([ii, jj]))
    ri, rj = np.searchsorted(u, ii), np.searchsorted(u, jj)
    assert be.sparse_plan(N, ri, rj)["nc"] > 0  # at the default (kDenseTailMin = 16)
    knobs("dense_tail_min", 0)
    assert be.sparse_plan(N, ri, rj)["nc"] == 0
