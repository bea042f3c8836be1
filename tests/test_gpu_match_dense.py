"""GPU checks of match_dense (mast3r_slam_backends.match_dense ->
m3s_match_dense, csrc/m3s_match.hip) and FactorGraph.add_factors_dense.

Two references:

* the composed path on the device, existing code only: ``matching.match``
  (prep_rays, iter_proj, torch occlusion test, refine_matches, pixel_to_lin),
  then the caller's glue, sqrt(Q11[b, idx] * Q21) and the count of
  valid & (Q > Q_conf) (global_opt.py:53-66). match_dense runs the same IEEE
  sequence, so idx, valid, n_valid and the bits of Q must be identical;
* the CPU oracle chain restated below in numpy: fusion_oracle.prep_rays,
  matching_oracle.iter_proj, the occlusion test in float64,
  matching_oracle.refine_matches, the Q combine in fp32. Pixels whose float64
  occlusion distance lies within 1e-5 of dist_thresh are left out (the fp32
  distance may fall on either side); their share must be <= 0.1%. On the rest
  idx and valid agree on >= 99% (the iter_proj bound of test_gpu_matching.py),
  and Q is bitwise equal wherever idx agrees.

Q11 / Q21 are uniform in [1, 3] from a seeded generator, Q_conf = 1.5.
"""
import functools

import numpy as np
import pytest
import torch

import mast3r_slam_backends as be
from mast3r_slam_amd import factor_graph as fgm
from mast3r_slam_amd import matching, synthetic
from oracle import fusion_oracle as fo
from oracle import matching_oracle as mo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CFG = matching.MATCHING_CFG
Q_CONF = 1.5


@functools.lru_cache(maxsize=None)
def _inputs(B, H, W, F=24, seed=1005):
    """CPU tensors (X11, X21, D11, D21, Q11, Q21, p_true) of B view pairs;
    never modified by a test."""
    ms = [synthetic.make_match_inputs(H, W, seed=seed + 17 * k, F=F) for k in range(B)]
    gen = torch.Generator().manual_seed(seed + 1)
    Q11 = 1.0 + 2.0 * torch.rand(B, H * W, generator=gen)
    Q21 = 1.0 + 2.0 * torch.rand(B, H * W, generator=gen)
    cat = lambda name: torch.cat([getattr(m, name) for m in ms]).contiguous()
    return cat("X11"), cat("X21"), cat("D11"), cat("D21"), Q11, Q21, cat("p_true")


def _dev(*ts):
    return [t.to(DEV) for t in ts]


def _glue(idx, valid, Q11, Q21, Q_conf=Q_CONF):
    """global_opt.py:53-66 on the outputs of matching.match."""
    B, HW = idx.shape
    bi = torch.arange(B, device=idx.device)[:, None].repeat(1, HW)
    Q = torch.sqrt(Q11.reshape(B, HW, 1)[bi, idx] * Q21.reshape(B, HW, 1))
    n = (valid & (Q > Q_conf)).sum(dim=(1, 2))
    return idx, valid, Q, n


def _composed(X11, X21, D11, D21, Q11, Q21, idx_init=None, cfg=CFG):
    idx, valid = matching.match(X11, X21, D11, D21, idx_init, cfg)
    return _glue(idx, valid, Q11, Q21)


def _composed_f32(X11, X21, D11, D21, Q11, Q21, cfg=CFG):
    """match_iterative_proj with float32 descriptors handed to refine_matches
    as they are (matching.match casts to half): the same entry points, by hand."""
    b, h, w = X21.shape[:3]
    img, pts, p0 = matching.prep_for_iter_proj(X11, X21)
    p1, conv = be.iter_proj(img, pts, p0, cfg["max_iter"], cfg["lambda_init"], cfg["convergence_thresh"])
    p1 = p1.long()
    bi = torch.arange(b, device=X11.device)[:, None].repeat(1, h * w)
    d = torch.linalg.norm(X11[bi, p1[..., 1], p1[..., 0], :].reshape(b, h, w, 3) - X21, dim=-1)
    valid = conv & (d < cfg["dist_thresh"]).view(b, -1)
    (p1,) = be.refine_matches(D11, D21.reshape(b, h * w, -1), p1.contiguous(), cfg["radius"], cfg["dilation_max"])
    return _glue(matching.pixel_to_lin(p1, w), valid.unsqueeze(-1), Q11, Q21)


def _assert_same(got, ref):
    idx, valid, Q, n = got
    ridx, rvalid, rQ, rn = ref
    assert idx.dtype == torch.int32 and valid.dtype == torch.bool and Q.dtype == torch.float32
    assert n.dtype == torch.int32
    assert idx.shape == ridx.shape and valid.shape == rvalid.shape and Q.shape == rQ.shape
    assert torch.equal(idx.long(), ridx)
    assert torch.equal(valid, rvalid)
    assert torch.equal(Q.view(torch.int32), rQ.view(torch.int32))  # bitwise
    assert torch.equal(n.long(), rn.long())


def _recount(idx, valid, Q):
    return (valid & (Q > Q_CONF)).sum(dim=(1, 2))


CASES = [(2, 37, 53), (1, 48, 64)]  # a wave straddling the batch elements, HW % 64 != 0 != HW % 256; one pair


@pytest.mark.parametrize("B,H,W", CASES)
def test_equals_composed_path(B, H, W):
    X11, X21, D11, D21, Q11, Q21 = _dev(*_inputs(B, H, W)[:6])
    got = be.match_dense(X11, X21, D11, D21, Q11, Q21, Q_conf=Q_CONF)
    ref = _composed(X11, X21, D11, D21, Q11, Q21)
    _assert_same(got, ref)
    frac = got[1].float().mean().item()
    assert 0.2 < frac < 0.9, frac  # both values of valid well represented
    same = matching.match_dense(X11, X21, D11, D21, Q11, Q21)  # the thin mirror: MATCHING_CFG defaults
    _assert_same(same, ref)


@functools.lru_cache(maxsize=None)
def _oracle_chain(B, H, W):
    """(idx, valid, Q, occlusion distance float64) of the CPU oracle chain."""
    X11, X21, D11, D21, Q11, Q21, _ = (t.numpy() for t in _inputs(B, H, W))
    HW = H * W
    img, pts = fo.prep_rays(X11, X21)
    img, pts = np.asarray(img), np.asarray(pts)
    ar = np.arange(HW)
    p0 = np.broadcast_to(np.stack((ar % W, ar // W), -1).astype(np.float32)[None], (B, HW, 2)).copy()
    p, conv = mo.iter_proj(img, pts, p0, CFG["max_iter"], CFG["lambda_init"], CFG["convergence_thresh"])
    p = p.astype(np.int64)  # .long()
    bi = np.arange(B)[:, None]
    diff = X11[bi, p[..., 1], p[..., 0]].astype(np.float64) - X21.reshape(B, HW, 3).astype(np.float64)
    dist = np.sqrt((diff * diff).sum(-1))
    valid = conv & (dist < CFG["dist_thresh"])
    p = mo.refine_matches(D11, D21.reshape(B, HW, -1), p, CFG["radius"], CFG["dilation_max"])
    idx = p[..., 0] + W * p[..., 1]
    Q = np.sqrt(Q11[bi, idx] * Q21)  # float32 multiply, float32 square root
    assert Q.dtype == np.float32
    return idx, valid, Q, dist


@pytest.mark.parametrize("B,H,W", CASES)
def test_against_cpu_oracle_chain(B, H, W):
    ridx, rvalid, rQ, dist = _oracle_chain(B, H, W)
    assert 0.25 < rvalid.mean() < 0.75, rvalid.mean()  # a constant output cannot pass
    X11, X21, D11, D21, Q11, Q21 = _dev(*_inputs(B, H, W)[:6])
    idx, valid, Q, n = be.match_dense(X11, X21, D11, D21, Q11, Q21, Q_conf=Q_CONF)
    assert torch.equal(n.long(), _recount(idx, valid, Q))  # the kernel's count of its own outputs, exactly
    idx, valid, Q = idx.cpu().numpy(), valid.cpu().numpy()[..., 0], Q.cpu().numpy()[..., 0]
    clear = np.abs(dist - CFG["dist_thresh"]) > 1e-5
    left_out = 1.0 - clear.mean()
    agree = ((idx == ridx) & (valid == rvalid))[clear].mean()
    print(f"{B}x{H}x{W}: left out {left_out:.5f}, idx & valid agree on {agree:.5f}")
    assert left_out <= 1e-3
    assert agree >= 0.99
    m = clear & (idx == ridx)
    assert np.array_equal(Q[m].view(np.int32), rQ[m].view(np.int32))


# At 3 x 3 base.yaml's thresholds leave no pixel valid (the CPU oracle chain
# agrees), so a count that never counted would pass; the loose thresholds make
# nearly every pixel valid, and the count of a batch element is then the number
# of its nine pixels with Q > Q_conf.
LOOSE = dict(CFG, convergence_thresh=1e3, dist_thresh=1e3)


@pytest.mark.parametrize("cfg", [CFG, LOOSE], ids=["base", "loose"])
@pytest.mark.parametrize("B", [3, 8])
def test_tiny_images_one_wave_spans_many_batch_elements(B, cfg):
    """3 x 3 is the smallest image m3s_iter_proj takes, N = 9. B = 3: one wave
    holds all 27 pixels of the three batch elements. B = 8: the first wave
    holds seven whole batch elements and one pixel of the eighth, the second
    wave the rest of the eighth."""
    X11, X21, D11, D21, Q11, Q21 = _dev(*_inputs(B, 3, 3)[:6])
    got = matching.match_dense(X11, X21, D11, D21, Q11, Q21, cfg=cfg, Q_conf=Q_CONF)
    assert torch.equal(got[3].long(), _recount(*got[:3]))
    if cfg is LOOSE:
        assert got[1].float().mean() > 0.5 and int(got[3].min()) > 0, got[3]
    _assert_same(got, _composed(X11, X21, D11, D21, Q11, Q21, cfg=cfg))


def test_idx_init():
    B, H, W = 2, 37, 53
    ins = _inputs(B, H, W)
    gen = torch.Generator().manual_seed(7)
    p = ins[6] + torch.randint(-3, 4, ins[6].shape, generator=gen)
    p[..., 0].clamp_(0, W - 1)
    p[..., 1].clamp_(0, H - 1)
    init = (p[..., 0] + W * p[..., 1]).contiguous().to(DEV)
    X11, X21, D11, D21, Q11, Q21 = _dev(*ins[:6])
    got = be.match_dense(X11, X21, D11, D21, Q11, Q21, init, Q_conf=Q_CONF)
    ref = _composed(X11, X21, D11, D21, Q11, Q21, init)
    _assert_same(got, ref)
    plain = be.match_dense(X11, X21, D11, D21, Q11, Q21, Q_conf=Q_CONF)
    assert not torch.equal(plain[0], got[0])  # the start pixel is used


def test_generic_refine_kernel_odd_feature_width():
    X11, X21, D11, D21, Q11, Q21 = _dev(*_inputs(2, 24, 32, F=20)[:6])
    got = be.match_dense(X11, X21, D11, D21, Q11, Q21, Q_conf=Q_CONF)
    _assert_same(got, _composed(X11, X21, D11, D21, Q11, Q21))


def test_float32_descriptors_at_the_c_level():
    """M3S_DESC_F32: the wrapper casts to half like the reference's caller, so
    float32 descriptors reach the library only through the checked call
    underneath it."""
    X11, X21, D11, D21, Q11, Q21 = _dev(*_inputs(2, 24, 32)[:6])
    D11, D21 = D11.float(), D21.float()
    got = be._match_dense(X11, X21, D11, D21, Q11, Q21, None, CFG["max_iter"], CFG["lambda_init"],
                          CFG["convergence_thresh"], CFG["dist_thresh"], CFG["radius"], CFG["dilation_max"],
                          Q_CONF, None)
    _assert_same(got, _composed_f32(X11, X21, D11, D21, Q11, Q21))


def test_radius_zero_skips_refinement():
    X11, X21, D11, D21, Q11, Q21 = _dev(*_inputs(2, 24, 32)[:6])
    cfg = dict(CFG, radius=0)
    got = matching.match_dense(X11, X21, D11, D21, Q11, Q21, cfg=cfg, Q_conf=Q_CONF)
    _assert_same(got, _composed(X11, X21, D11, D21, Q11, Q21, cfg=cfg))
    refined = matching.match_dense(X11, X21, D11, D21, Q11, Q21, Q_conf=Q_CONF)
    assert not torch.equal(refined[0], got[0])


def test_strided_destination():
    """out= views of a [2*cap, HW] store at rows r0:r1:2; the rows in between
    keep their sentinel."""
    B, H, W = 2, 37, 53
    HW, cap, r0 = H * W, 4, 3
    r1 = r0 + 2 * B
    X11, X21, D11, D21, Q11, Q21 = _dev(*_inputs(B, H, W)[:6])
    ref = be.match_dense(X11, X21, D11, D21, Q11, Q21, Q_conf=Q_CONF)
    idx = torch.full((2 * cap, HW), -7, dtype=torch.int32, device=DEV)
    vraw = torch.full((2 * cap, HW, 1), 0xAB, dtype=torch.uint8, device=DEV)
    Q = torch.full((2 * cap, HW, 1), -3.0, device=DEV)
    valid = vraw.view(torch.bool)
    rows = slice(r0, r1, 2)
    got = be.match_dense(X11, X21, D11, D21, Q11, Q21, Q_conf=Q_CONF, out=(idx[rows], valid[rows], Q[rows]))
    assert got[0].data_ptr() == idx[rows].data_ptr()
    assert torch.equal(idx[rows], ref[0]) and torch.equal(Q[rows], ref[2])
    assert torch.equal(vraw[rows], ref[1].view(torch.uint8))
    assert torch.equal(got[3], ref[3])
    other = torch.ones(2 * cap, dtype=torch.bool, device=DEV)
    other[rows] = False
    assert (idx[other] == -7).all() and (vraw[other] == 0xAB).all() and (Q[other] == -3.0).all()


def _edge_inputs(H, W, e):
    """Decoder outputs of e undirected edges: the i->j half and the j->i half
    of the symmetric batch, each from its own seeded view pairs."""
    fwd, rev = _inputs(e, H, W, seed=2000), _inputs(e, H, W, seed=3000)
    shape = lambda t: t.reshape(e, H, W, -1).contiguous()
    Xii, Xji, Dii, Dji, Qii, Qji = fwd[:6]
    Xjj, Xij, Djj, Dij, Qjj, Qij = rev[:6]
    Qii, Qji, Qjj, Qij = Qii.clone(), Qji.clone(), Qjj.clone(), Qij.clone()
    for k in (0, 1):  # edges 0 and 1: every combined Q <= 0.9 < Q_conf -> match fraction 0
        for q in (Qii, Qji, Qjj, Qij):
            q[k] *= 0.3
    return _dev(Xii, shape(Xji), Xjj, shape(Xij), Dii, shape(Dji), Djj, shape(Dij),
                Qii.reshape(e, H, W), Qji.reshape(e, H, W), Qjj.reshape(e, H, W), Qij.reshape(e, H, W))


def test_add_factors_dense_equals_add_factors_on_composed_path():
    """Three undirected edges at 24 x 32: (0,1) consecutive with match fraction
    0 (exempt), (0,2) with match fraction 0 (dropped), (0,3) good. The edge
    store starts with capacity 2, so the call also grows it."""
    H, W, e = 24, 32, 3
    ii, jj = [0, 0, 0], [1, 2, 3]
    Xii, Xji, Xjj, Xij, Dii, Dji, Djj, Dij, Qii, Qji, Qjj, Qij = _edge_inputs(H, W, e)
    flat = lambda q: q.reshape(e, H * W)
    i2j, vj, Qj, nj = _composed(Xii, Xji, Dii, Dji, flat(Qii), flat(Qji))
    j2i, vi, Qi, ni = _composed(Xjj, Xij, Djj, Dij, flat(Qjj), flat(Qij))
    assert nj[0] == 0 and nj[1] == 0 and min(int(nj[2]), int(ni[2])) > 0.1 * H * W
    ref = fgm.FactorGraph(fgm.KeyframeStore(H, W, DEV, capacity=4), edge_capacity=2)
    assert ref.add_factors(ii, jj, i2j, j2i, vj, vi, Qj, Qi, 0.1) is True
    fg = fgm.FactorGraph(fgm.KeyframeStore(H, W, DEV, capacity=4), edge_capacity=2)
    args = (ii, jj, Xii, Xji, Xjj, Xij, Dii, Dji, Djj, Dij, Qii, Qji, Qjj, Qij)
    assert fg.add_factors_dense(*args, 0.1) is True
    assert fg.edges.n == ref.edges.n == 2
    for got, want in zip(fg.edges.directed(), ref.edges.directed()):
        assert got.dtype == want.dtype and torch.equal(got, want)
    assert torch.equal(fg.ii_u, ref.ii_u) and torch.equal(fg.jj_u, ref.jj_u)
    assert fg.ii_u.tolist() == [0, 0] and fg.jj_u.tolist() == [1, 3]
    # a second call appends after the first
    assert fg.add_factors_dense(*args, 0.1) is True and ref.add_factors(ii, jj, i2j, j2i, vj, vi, Qj, Qi, 0.1)
    for got, want in zip(fg.edges.directed(), ref.edges.directed()):
        assert torch.equal(got, want)
    # relocalisation: any rejected edge rejects the call
    assert fg.add_factors_dense(*args, 0.1, is_reloc=True) is False
    assert fg.edges.n == 4 and fg.ii_u.numel() == 4


def test_bad_inputs_raise():
    X11, X21, D11, D21, Q11, Q21 = _dev(*_inputs(2, 24, 32)[:6])
    HW = 24 * 32
    with pytest.raises(RuntimeError, match="contiguous"):
        be.match_dense(X11.transpose(1, 2), X21, D11, D21, Q11, Q21)
    with pytest.raises(RuntimeError, match="Q11"):
        be.match_dense(X11, X21, D11, D21, Q11[:, :-1].contiguous(), Q21)
    with pytest.raises(RuntimeError, match="ROCm device"):
        be.match_dense(X11, X21.cpu(), D11, D21, Q11, Q21)
    out = (torch.empty(2, HW - 1, dtype=torch.int32, device=DEV),
           torch.empty(2, HW, 1, dtype=torch.bool, device=DEV), torch.empty(2, HW, 1, device=DEV))
    with pytest.raises(RuntimeError, match="out idx"):
        be.match_dense(X11, X21, D11, D21, Q11, Q21, out=out)
