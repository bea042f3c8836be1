"""This project's own statement of the 2-D rotary position embedding that
m3s_rope_2d computes (include/m3s_rope.h), for the tests and the timing tool.

One head row of D = 4 Q channels is [u_Y(Q) | v_Y(Q) | u_X(Q) | v_X(Q)]; for the
axis a in {Y, X} and the frequency index i in [0, Q):

    theta = pos[b, n, a] * F0 / base^(i/Q)
    u'    = u cos(theta) - v sin(theta)
    v'    = v cos(theta) + u sin(theta)

rope2d_exact  evaluates that in fp64 (torch ops, differentiable).
bound         is the derived per-element tolerance of an fp32 evaluation.
rope2d_torch  is a plain-torch fp-as-given implementation with the cost profile
              of what a ROCm user of the reference runs today (tools/rope_time.py).

Tokens are [B, H, N, D] and positions [B, N, 2] int64 (y, x) throughout, as the
attention blocks pass them.
"""
import torch

EPS32 = 2.0 ** -24  # unit roundoff of fp32


def _pairs(x):
    """[B, H, N, D] -> (u, v), each [B, H, N, 2 (axis), Q]."""
    B, H, N, D = x.shape
    x = x.reshape(B, H, N, 2, 2, D // 4)
    return x[..., 0, :], x[..., 1, :]


def rope2d_exact(tokens, pos, base, F0):
    """The function above in fp64 on the given inputs (tokens of any float
    dtype are widened exactly); -> fp64 [B, H, N, D]."""
    t = tokens.to(torch.float64)
    B, H, N, D = t.shape
    assert D % 4 == 0 and tuple(pos.shape) == (B, N, 2)
    Q = D // 4
    i = torch.arange(Q, dtype=torch.float64, device=t.device)
    freq = float(F0) / torch.pow(torch.tensor(float(base), dtype=torch.float64, device=t.device), i / Q)
    theta = pos.to(torch.float64)[..., None] * freq  # [B, N, 2, Q]
    c, s = theta.cos()[:, None], theta.sin()[:, None]
    u, v = _pairs(t)
    return torch.stack((u * c - v * s, v * c + u * s), dim=-2).reshape(B, H, N, D)


def bound(tokens, pmax, F0):
    """Per-element tolerance |fp32 evaluation - exact| <= (12 pmax |F0| + 7) eps
    (|u| + |v|), eps = 2^-24, for base <= 100 and |pos| <= pmax < 2^24; fp64
    [B, H, N, D]. Derived, not measured:

    theta. (float)pos is exact. x = fl(i/Q) has relative error eps and x < 1, so
    base^x moves by a relative ln(base) x eps <= 4.6 eps; powf is within 2 ulp
    = 4 eps; the division and the product are correctly rounded, eps each. The
    relative error of theta is at most 10.6 eps, taken as 12 eps; base^x >= 1, so
    |theta| <= pmax |F0| and |d theta| <= 12 pmax |F0| eps.

    cos, sin. Both have slope at most 1, so they move by at most |d theta|;
    sincosf is within 2 ulp of values <= 1, at most 4 eps absolute.

    rotation. u' = fl(fl(u c) - fl(v s)): eps per product and eps for the sum,
    each on at most |u| + |v|, taken as 3 eps (|u| + |v|).

    The errors of cos and sin enter u' and v' multiplied by |u| and |v|, so the
    sum is (12 pmax |F0| + 4 + 3) eps (|u| + |v|)."""
    return (12.0 * float(pmax) * abs(float(F0)) + 7.0) * EPS32 * pair_sum(tokens)


def pair_sum(tokens):
    """|u| + |v| of the pair every element belongs to; fp64 [B, H, N, D]."""
    u, v = _pairs(tokens.to(torch.float64).abs())
    a = u + v
    return torch.stack((a, a), dim=-2).reshape(tokens.shape)


def ulp(x, dtype):
    """The spacing of `dtype` at the binade of each |x| (fp64 in, fp64 out),
    the subnormal spacing below the smallest normal."""
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}[dtype]
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** emin)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=x.device), e - mant)


_TABLES = {}


def rope2d_torch(tokens, positions, base=100.0, F0=1.0):
    """Plain torch, in the tokens' dtype, out of place: cos / sin tables over the
    positions 0 .. max (kept between calls), rows looked up with `embedding`,
    rotate-half by concatenation. The table length comes from
    int(positions.max()), a host read on every call: this is the work a ROCm
    user's forward pass does per q and per k today."""
    B, H, N, D = tokens.shape
    half = D // 2
    length = int(positions.max()) + 1
    key = (half, length, tokens.device, tokens.dtype, float(base), float(F0))
    if key not in _TABLES:
        freq = float(F0) / (float(base) ** (torch.arange(0, half, 2, device=tokens.device).float() / half))
        ang = (torch.arange(length, device=tokens.device).float()[:, None] * freq[None, :]).to(tokens.dtype)
        ang = torch.cat((ang, ang), dim=-1)
        _TABLES[key] = (ang.cos(), ang.sin())
    cos, sin = _TABLES[key]
    out = []
    for axis, part in enumerate(tokens.chunk(2, dim=-1)):
        c = torch.nn.functional.embedding(positions[:, :, axis], cos)[:, None]
        s = torch.nn.functional.embedding(positions[:, :, axis], sin)[:, None]
        a, b = part[..., : half // 2], part[..., half // 2:]
        out.append(part * c + torch.cat((-b, a), dim=-1) * s)
    return torch.cat(out, dim=-1)
