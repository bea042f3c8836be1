"""GPU check of the edge-sharded GN path (mast3r_slam_amd/distributed.py over
the stepwise C ABI m3s_gn_prepare / m3s_gn_linearize / m3s_gn_solve) that
bench.py runs at N > 1 GPUs.

One process, one GPU: R "ranks" are R HipOps instances, each with its own
workspace, pose tensor and edge slice; the all-gather of the per-edge normal
equations is a torch.cat. Every rank must end with bitwise-identical poses
(identical inputs, deterministic kernels: nothing is broadcast in the real
run), and the poses must match the single-call gauss_newton_* entry point
(different reduction grouping: fused per-edge finalize vs edge_reduce, same
tolerance as the oracle tests) and the CPU oracle.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def be():
    import mast3r_slam_backends as be

    return be


def sharded_solve(be, mode, g, Xs, world, iters, delta, sig, idx_dtype=torch.int64):
    """Pair-preserving shards (distributed.edge_shard), the solve on the
    payload-ordered edge list (distributed.payload_ids) as ShardedGN runs it."""
    from mast3r_slam_amd.distributed import HipOps, edge_shard, payload_ids

    E = g.n_edges
    ii_p, jj_p = payload_ids(g.ii.to(DEV), g.jj.to(DEV), world)
    ranks = []
    for r in range(world):
        ids, per = edge_shard(E, r, world)
        Twc = g.T_init.data.clone().to(DEV).contiguous()
        ops = HipOps(mode, Twc, Xs, g.Cs.to(DEV).contiguous(), ii_p, jj_p,
                     g.idx_ii2jj[ids].to(DEV).to(idx_dtype).contiguous(), g.valid_match[ids].to(DEV).contiguous(),
                     g.Q[ids].to(DEV).contiguous(), len(ii_p), g.K.to(DEV) if mode == be.MODE_CALIB else None,
                     **sig)
        es = torch.zeros(per, ops.stride, dtype=torch.float64, device=DEV)
        ranks.append((r * per, r * per + len(ids), per, Twc, ops, es))
    for *_, ops, _ in ranks:
        ops.prepare(delta)
    for _ in range(iters):
        for eb, ee, per, Twc, ops, es in ranks:
            if ee > eb:
                ops.linearize(eb, ee, es)
        es_all = torch.cat([es for *_, es in ranks])  # the all_gather_into_tensor payload
        for *_, ops, _ in ranks:
            ops.solve(es_all)
    torch.cuda.synchronize()
    return [Twc.cpu().numpy() for _, _, _, Twc, _, _ in ranks], [ops.info.cpu().numpy() for *_, ops, _ in ranks]


@pytest.mark.parametrize("mode,world", [("rays", 2), ("calib", 3), ("calib", 2)])
def test_sharded_ranks_agree_and_match_single_call(be, mode, world):
    from mast3r_slam_amd import synthetic

    g = synthetic.make_graph(7, 48, 64, seed=41)
    if mode == "calib":
        rays = synthetic.pixel_rays(g.H, g.W, g.K)
        Xs = (g.Xs[..., 2:3] * rays[None]).to(DEV).contiguous()
        sig = dict(sigma_a=1.0, sigma_b=10.0, C_thresh=0.0, Q_thresh=1.5, height=g.H, width=g.W,
                   pixel_border=-10, z_eps=1e-6)
        m = be.MODE_CALIB
    else:
        Xs = g.Xs.to(DEV).contiguous()
        sig = dict(sigma_a=0.003, sigma_b=10.0, C_thresh=0.0, Q_thresh=1.5)
        m = be.MODE_RAYS
    iters = 5
    poses, infos = sharded_solve(be, m, g, Xs, world, iters, 0.0, sig)
    for r in range(1, world):
        np.testing.assert_array_equal(poses[r], poses[0])
    for inf in infos:
        assert int(inf[be.INFO_ITERS]) == iters

    Twc = g.T_init.data.clone().to(DEV).contiguous()
    info = torch.zeros(8, dtype=torch.int32, device=DEV)
    args = [t.to(DEV).contiguous() for t in (g.Cs, g.ii, g.jj, g.idx_ii2jj, g.valid_match, g.Q)]
    if mode == "calib":
        Cs, ii, jj, idx, valid, Q = args
        be.gauss_newton_calib(Twc, Xs, Cs, g.K.to(DEV), ii, jj, idx, valid, Q, g.H, g.W, -10, 1e-6,
                              1.0, 10.0, 0.0, 1.5, iters, 0.0, info=info)
    else:
        Cs, ii, jj, idx, valid, Q = args
        be.gauss_newton_rays(Twc, Xs, Cs, ii, jj, idx, valid, Q, 0.003, 10.0, 0.0, 1.5, iters, 0.0,
                             info=info)
    torch.cuda.synchronize()
    ref = Twc.cpu().numpy()
    # fp32 per-pixel sums grouped differently (edge_reduce vs the fused
    # per-edge finalize); cond(H) amplifies it: DESIGN.md §5 pose tolerance
    np.testing.assert_allclose(poses[0], ref, rtol=0, atol=1e-4)
    assert not np.array_equal(poses[0], g.T_init.data.numpy())  # the solve moved the poses


def test_sharded_natural_termination(be):
    """delta > 0: the device stop flag ends every rank after the same step."""
    from mast3r_slam_amd import synthetic

    g = synthetic.make_graph(5, 32, 48, seed=43)
    sig = dict(sigma_a=0.003, sigma_b=10.0, C_thresh=0.0, Q_thresh=1.5)
    poses, infos = sharded_solve(be, be.MODE_RAYS, g, g.Xs.to(DEV).contiguous(), 2, 20, 1e-3, sig)
    np.testing.assert_array_equal(poses[0], poses[1])
    its = [int(i[be.INFO_ITERS]) for i in infos]
    assert its[0] == its[1] < 20
    assert all(int(i[be.INFO_CONVERGED]) == 1 for i in infos)


def test_sharded_int32_idx_matches_int64(be):
    """HipOps with the device edge store's int32 match indices (factor_graph
    EdgeStore): idx_i32 is set for the C side, so the gathering linearize
    reads 4-B ids; the poses are bitwise those of the int64 run."""
    from mast3r_slam_amd import synthetic

    g = synthetic.make_graph(7, 48, 64, seed=41)
    sig = dict(sigma_a=0.003, sigma_b=10.0, C_thresh=0.0, Q_thresh=1.5)
    Xs = g.Xs.to(DEV).contiguous()
    p64, i64 = sharded_solve(be, be.MODE_RAYS, g, Xs, 2, 4, 0.0, sig)
    p32, i32 = sharded_solve(be, be.MODE_RAYS, g, Xs, 2, 4, 0.0, sig, idx_dtype=torch.int32)
    for a, b in zip(p64, p32):
        np.testing.assert_array_equal(a, b)
    assert all(int(i[be.INFO_SOLVE_FAIL]) == 0 for i in i32)


def test_stepwise_edge_sums_fused_reduce_across_ranges(be):
    """The stepwise linearize writes each edge's fp64 sums from the edge's
    last chunk (the per-edge arrival counters run on over a call's launches;
    a range change re-zeroes them). Changing ranges on one workspace must
    give bitwise the sums of fresh workspaces running the same launches."""
    from mast3r_slam_amd import synthetic
    from mast3r_slam_amd.distributed import HipOps

    g = synthetic.make_graph(7, 48, 64, seed=41)
    sig = dict(sigma_a=0.003, sigma_b=10.0, C_thresh=0.0, Q_thresh=1.5)
    Xs = g.Xs.to(DEV).contiguous()
    E = g.n_edges
    eb, ee = 0, 4  # (the stepwise API addresses edge data from the range start: ranges from 0 here)

    def run(seq):
        Twc = g.T_init.data.clone().to(DEV).contiguous()
        ops = HipOps(be.MODE_RAYS, Twc, Xs, g.Cs.to(DEV).contiguous(), g.ii.to(DEV), g.jj.to(DEV),
                     g.idx_ii2jj.to(DEV).contiguous(), g.valid_match.to(DEV).contiguous(),
                     g.Q.to(DEV).contiguous(), E, None, **sig)
        ops.prepare(0.0)
        out = []
        for b, e in seq:
            es = torch.full((e - b, ops.stride), float("nan"), dtype=torch.float64, device=DEV)
            ops.linearize(b, e, es)
            out.append(es)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in out]

    A1, A2 = run([(0, E), (0, E)])  # gathering launch, then packed
    C1, C2 = run([(eb, ee), (eb, ee)])
    S1, S2, B1, B2, S3 = run([(eb, ee), (eb, ee), (0, E), (0, E), (eb, ee)])
    for x, y in ((S1, C1), (S2, C2), (B1, A1), (B2, A2), (S3, C1)):
        assert np.isfinite(x).all()
        np.testing.assert_array_equal(x, y)
    # the sub-range's sums are the same edges' sums (other chunking: fp32
    # partials grouped differently)
    np.testing.assert_allclose(S1, A1[eb:ee], rtol=1e-4, atol=1e-6 * np.abs(A1).max())


def test_stepwise_host_prepare_cache_hit_starts_from_fresh_call_state(be, knobs):
    """A plan-cache entry is a plan, not the call that built it. Host prepare
    (knob prologue = 0), 48x64: 3 chunks per edge, not a power of two. Call 1
    caches its plan at its first solve, after a linearize with edge sums has
    counted arrivals; call 2 on a fresh workspace hits the cache at prepare and
    must count its arrivals from its own zeroed counters: its edge sums are
    finite and bitwise those of call 1. With an arrival count inherited from
    the cached call, the wrong chunk of an edge would write the edge's sums
    (the second arrival of three; it reads the third chunk's partial, which
    is usually stored by then, so that fault shows only when timing allows).
    The same with the cache off for call 2 (a miss: the plan is deferred)."""
    from mast3r_slam_amd import synthetic
    from mast3r_slam_amd.distributed import HipOps

    knobs("prologue", 0)
    g = synthetic.make_graph(7, 48, 64, seed=41)
    sig = dict(sigma_a=0.003, sigma_b=10.0, C_thresh=0.0, Q_thresh=1.5)
    Xs = g.Xs.to(DEV).contiguous()
    E = g.n_edges

    def call(solve):
        Twc = g.T_init.data.clone().to(DEV).contiguous()
        ops = HipOps(be.MODE_RAYS, Twc, Xs, g.Cs.to(DEV).contiguous(), g.ii.to(DEV), g.jj.to(DEV),
                     g.idx_ii2jj.to(DEV).contiguous(), g.valid_match.to(DEV).contiguous(),
                     g.Q.to(DEV).contiguous(), E, None, **sig)
        ops.ws.zero_()
        ops.prepare(0.0)
        es = torch.full((E, ops.stride), float("nan"), dtype=torch.float64, device=DEV)
        ops.linearize(0, E, es)
        if solve:
            ops.solve(es)
        torch.cuda.synchronize()
        ops.close()
        return es.cpu().numpy()

    for cache2 in (1, 0):
        # a plan-shaping knob set to another value drops the plan cache: call 1 starts cold
        be.set_knob("dense_tail_min", be.set_knob("dense_tail_min", 1 << 20))
        knobs("plan_cache", 1)
        es1 = call(True)
        knobs("plan_cache", cache2)
        es2 = call(False)
        assert np.isfinite(es1).all() and np.isfinite(es2).all()
        np.testing.assert_array_equal(es2, es1)
