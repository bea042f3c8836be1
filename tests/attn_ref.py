"""This project's own statement of the attention core that m3s_attn_rope
computes (include/m3s_attn.h), for the tests and the timing tool.

    out[b,i,h,:] = sum_j softmax_j(scale <R(q[b,i,h], qpos[b,i]), R(k[b,j,h], kpos[b,j])>) v[b,j,h,:]

with R the rotation of tests/rope_ref.py; positions None = no rotation.

attn_exact   evaluates that in fp64 (torch ops).
attn_torch   is the reference's plain-torch statement (croco blocks.py:94-112,
             149-169) in the dtype given, with the rope passed in.
bound        is the derived per-element tolerance of an fp32 evaluation.
load_fixture reads tests/golden/attn_{a..d}.npz (make_attn_golden.py).
RoPE2D, Attention, CrossAttention are stand-ins with the reference's class and
attribute names (croco models/blocks.py), for attention.install.

q [B, Nq, H, D], k and v [B, Nk, H, D] throughout, as the kernel takes them;
results are [B, Nq, H * D], as `proj` takes them.
"""
import os

import numpy as np
import torch

import rope_ref

EPS32 = rope_ref.EPS32
TILE = 32  # kv rows per step of the running softmax
D = 64  # the head dimension of every fixture


def load_fixture(golden_dir, name, device="cpu"):
    """-> dict(q, k, v [B,N,H,D] views, qpos, kpos, out, base, F0, scale, pmax, kind, qkv or None)."""
    z = np.load(os.path.join(golden_dir, f"attn_{name}.npz"))
    H = int(z["H"])
    c = dict(kind=str(z["kind"]), H=H, base=float(z["base"]), F0=float(z["F0"]), scale=float(z["scale"]),
             pmax=int(z["pmax"]), out=torch.from_numpy(z["out"]).to(device), qkv=None)
    if c["kind"] == "self":
        qkv = torch.from_numpy(z["qkv"]).to(device)
        B, N, _ = qkv.shape
        c["qkv"] = qkv.view(B, N, 3, H, D)
        c["q"], c["k"], c["v"] = (c["qkv"][:, :, i] for i in range(3))  # the real qkv-slice views
        c["qpos"] = c["kpos"] = torch.from_numpy(z["pos"]).to(device)
    else:
        for n in ("q", "k", "v"):
            t = torch.from_numpy(z[n]).to(device)
            c[n] = t.view(t.shape[0], t.shape[1], H, D)
        c["qpos"], c["kpos"] = torch.from_numpy(z["qpos"]).to(device), torch.from_numpy(z["kpos"]).to(device)
    return c


def call_args(c):
    return c["q"], c["k"], c["v"], c["qpos"], c["kpos"], c["base"], c["F0"], c["scale"]


def _rot(t, pos, base, F0):
    """fp64 [B, H, N, D] of a [B, N, H, D] tensor, rotated when pos is given."""
    t = t.to(torch.float64).permute(0, 2, 1, 3)
    return t if pos is None else rope_ref.rope2d_exact(t, pos, base, F0)


def attn_parts(q, k, v, qpos, kpos, base, F0, scale):
    """fp64 (q' [B,H,Nq,D], k' [B,H,Nk,D], v [B,H,Nk,D], scores [B,H,Nq,Nk], p)."""
    qr, kr = _rot(q, qpos, base, F0), _rot(k, kpos, base, F0)
    s = (qr @ kr.transpose(-2, -1)) * float(scale)
    return qr, kr, v.to(torch.float64).permute(0, 2, 1, 3), s, torch.softmax(s, dim=-1)


def _merge(x):
    """[B, H, N, D] -> [B, N, H * D]."""
    B, H, N, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, N, H * D)


def attn_exact(q, k, v, qpos, kpos, base, F0, scale):
    """The function above in fp64 on the given inputs; -> fp64 [B, Nq, H * D]."""
    _, _, vv, _, p = attn_parts(q, k, v, qpos, kpos, base, F0, scale)
    return _merge(p @ vv)


def attn_torch(q, k, v, qpos, kpos, scale, rope=None):
    """Statement (a): the reference's lines on [B, H, N, D] views, in the dtype
    given; `rope(tokens [B,H,N,D], pos)` may rotate in place, as the reference's
    does (pass clones to keep q and k)."""
    B, Nq, H, D = q.shape
    q, k, v = (t.transpose(1, 2) for t in (q, k, v))
    if rope is not None:
        q = rope(q, qpos)
        k = rope(k, kpos)
    attn = (q @ k.transpose(-2, -1)) * scale
    attn = attn.softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(B, Nq, H * D)


def rope_bound(tokens, pos, base, F0):
    """rope_ref.bound with its last step left out: that derivation shows the
    relative error of theta to be at most 12 eps, so |d theta| <= 12 eps
    |theta|, and only then replaces |theta| by its largest value pmax |F0|. Here
    every element keeps its own theta = pos * F0 / base^(i/Q): (12 |theta| + 7)
    eps (|u| + |v|); tokens [B, H, N, D], fp64 out."""
    B, H, N, D = tokens.shape
    Q = D // 4
    i = torch.arange(Q, dtype=torch.float64, device=tokens.device)
    freq = abs(float(F0)) / torch.pow(torch.tensor(float(base), dtype=torch.float64, device=tokens.device), i / Q)
    theta = pos.to(torch.float64).abs()[..., None] * freq  # [B, N, 2, Q]
    theta = torch.stack((theta, theta), dim=-2).reshape(B, 1, N, D)  # u and v of a pair share it
    return (12.0 * theta + 7.0) * EPS32 * rope_ref.pair_sum(tokens)


def bound(q, k, v, qpos, kpos, base, F0, scale):
    """Per-element tolerance |fp32 evaluation - attn_exact| of any evaluation
    that rotates as rope_ref.bound assumes, forms each score as a D-term fp32
    fmaf chain (or any fp32 sum of D rounded products), and runs the softmax
    with a running maximum over steps of TILE keys and an exp within 1 ulp;
    fp64 [B, Nq, H * D]. Derived, not measured; eps = 2^-24. First order in eps
    throughout; the second-order terms are covered by the final factor 1.01
    (every relative error here is < 1e-3).

    1. rope, propagated into the scores. rope_bound below gives |q^ - q'| <= rq =
    (12 |theta| + 7) eps (|u| + |v|) per element, likewise rk; without
    positions both are 0. The prescale q^ * scale rounds once: eps |q'|.
    So the score moves by scale * sum_d (rq |k'| + |q'| rk) + eps |scale| sum_d
    |q'| |k'|.

    2. the D-term chain. One rounding per fmaf, each on a partial sum bounded by
    sum_d |q'_d k'_d|: D eps |scale| sum_d |q'| |k'|. With 1: ds_ij = |scale|
    (sum_d (rq |k'| + |q'| rk) + (D + 1) eps sum_d |q'| |k'|).

    3. exp and the sums. out = sum_j w_j v_j / sum_j w_j is unchanged by a common
    factor on the w_j, so only relative errors between the weights count. The
    weight of key j is e^(s_j - m) built as a product of exps: its own, of
    fl(s_j - m_t) at the running maximum m_t of its step, and one rescale
    e^(m_t - m_t+1) per later step. Each subtraction rounds by eps times its
    size and the sizes add up to |s_j - m| (the maximum only grows); each exp is
    within 1 ulp <= 2 eps; each rescale multiplies once: eps. With T =
    ceil(Nk / TILE) steps and one more join, the relative error of w_j is
    eta_j = ds_ij + eps (|s_j - m| + 3 (T + 1) + 2).
    The two sums have at most Nk terms each plus the join: (Nk + 2) eps on sum_j
    p_j |v_jd| and on the normaliser, one division: eps. So

      |d out_d| <= sum_j p_j eta_j |v_jd| + |out_d| sum_j p_j eta_j
                   + (Nk + 3) eps (sum_j p_j |v_jd| + |out_d|)."""
    qr, kr, vv, s, p = attn_parts(q, k, v, qpos, kpos, base, F0, scale)
    D, Nk = q.shape[3], k.shape[1]
    scale = abs(float(scale))

    def moved(t, rotated, pos):  # [B, H, N, D] error of the rotated tensor
        return torch.zeros_like(rotated) if pos is None else rope_bound(t.permute(0, 2, 1, 3), pos, base, F0)

    rq, rk = moved(q, qr, qpos), moved(k, kr, kpos)
    aq, ak = qr.abs(), kr.abs()
    ds = scale * (rq @ ak.transpose(-2, -1) + aq @ rk.transpose(-2, -1)
                  + (D + 1) * EPS32 * (aq @ ak.transpose(-2, -1)))
    T = -(-Nk // TILE)
    eta = ds + EPS32 * ((s - s.amax(dim=-1, keepdim=True)).abs() + 3 * (T + 1) + 2)
    pe = p * eta
    av = vv.abs()
    out = (p @ vv).abs()
    b = pe @ av + out * pe.sum(dim=-1, keepdim=True) + (Nk + 3) * EPS32 * (p @ av + out)
    return 1.01 * _merge(b)


# ---- stand-ins with the reference's class and attribute names and tensor plumbing
class RoPE2D(torch.nn.Module):
    """rope_ref.rope2d_exact rounded once to the tokens' dtype, out of place."""

    def __init__(self, freq=100.0, F0=1.0):
        super().__init__()
        self.base, self.F0 = freq, F0

    def forward(self, tokens, positions):
        return rope_ref.rope2d_exact(tokens, positions, self.base, self.F0).to(tokens.dtype)


class Attention(torch.nn.Module):
    def __init__(self, dim, rope=None, num_heads=2, attn_drop=0.0):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = torch.nn.Linear(dim, dim * 3)
        self.attn_drop = torch.nn.Dropout(attn_drop)
        self.proj = torch.nn.Linear(dim, dim)
        self.proj_drop = torch.nn.Dropout(0.0)
        self.rope = rope

    def forward(self, x, xpos):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).transpose(1, 3)
        q, k, v = [qkv[:, :, i] for i in range(3)]
        if self.rope is not None:
            q, k = self.rope(q, xpos), self.rope(k, xpos)
        attn = self.attn_drop(((q @ k.transpose(-2, -1)) * self.scale).softmax(dim=-1))
        return self.proj_drop(self.proj((attn @ v).transpose(1, 2).reshape(B, N, C)))


class CrossAttention(torch.nn.Module):
    def __init__(self, dim, rope=None, num_heads=2):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.projq, self.projk, self.projv = (torch.nn.Linear(dim, dim) for _ in range(3))
        self.attn_drop = torch.nn.Dropout(0.0)
        self.proj = torch.nn.Linear(dim, dim)
        self.proj_drop = torch.nn.Dropout(0.0)
        self.rope = rope

    def forward(self, query, key, value, qpos, kpos):
        B, Nq, C = query.shape
        Nk, H = key.shape[1], self.num_heads
        q = self.projq(query).reshape(B, Nq, H, C // H).permute(0, 2, 1, 3)
        k = self.projk(key).reshape(B, Nk, H, C // H).permute(0, 2, 1, 3)
        v = self.projv(value).reshape(B, Nk, H, C // H).permute(0, 2, 1, 3)
        if self.rope is not None:
            q, k = self.rope(q, qpos), self.rope(k, kpos)
        attn = self.attn_drop(((q @ k.transpose(-2, -1)) * self.scale).softmax(dim=-1))
        return self.proj_drop(self.proj((attn @ v).transpose(1, 2).reshape(B, Nq, C)))
