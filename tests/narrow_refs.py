"""Plain torch restatements of the reference formulas behind the narrow-width row kernels (csrc/narrow.hip), shared by
test_hip_narrow.py and test_hip_narrow_walk.py: layers/global_message_passing.py:52-53, layers/local_message_passing.py:
46-49, layers/basic.py:25-33,74-76, models.py:185-188.

Every function computes in the dtype of the tensors it is given: fp64 operands give the reference the kernels are held
to, fp32 operands the plain-autograd figure that bounds what an fp32 sum over all rows can reach."""
import torch
import torch.nn.functional as F


def global_message(x1, P, e, wm, bm, wea, i, j):
    """x1 + sum_{q: tgt[q] = i} SiLU(P[i, :d] + P[src[q], d:] + e[q] We^T + b) * (e[q] Wea^T); We = wm[:, 2d:]."""
    n, d = x1.shape
    z = P[i, :d] + P[j, d:] + e @ wm[:, 2 * d:].t() + bm
    msg = F.silu(z) * (e @ wea.t())
    return x1 + torch.zeros(n, d, dtype=x1.dtype, device=x1.device).index_add_(0, i, msg)


def mlp2(x, w1, b1, w2, b2, res_x=False, r=None):
    """SiLU(W2 SiLU(W1 x + b1) + b2) [+ x] [+ r]."""
    y = F.silu(F.linear(F.silu(F.linear(x, w1, b1)), w2, b2))
    if res_x:
        y = y + x
    if r is not None:
        y = y + r
    return y


def linear(x, w, b, act=True):
    y = F.linear(x, w, b)
    return F.silu(y) if act else y


def project4(x, wj, wk):
    """The four node-side projections of two 3d-wide message weights: blocks (wj, 0), (wk, 0), (wj, d), (wk, d)."""
    d = x.size(1)
    return F.linear(x, torch.cat([wj[:, :d], wk[:, :d], wj[:, d:2 * d], wk[:, d:2 * d]], 0))


def embed(f, kind, wa, ba, wb=None, bb=None):
    """SiLU(W f + b); with `kind`, rows of kind 0 use (wa, ba) and the others (wb, bb)."""
    ya = F.silu(F.linear(f, wa, ba))
    if kind is None:
        return ya
    yb = F.silu(F.linear(f, wb, bb))
    return torch.where(kind.bool().unsqueeze(1), yb, ya)


def embed_rbf(dist, freq, w, b, cutoff):
    """SiLU(W (u(x) sin(f x)) + b), x = dist / cutoff, u the p = 5 envelope (zero from the cutoff on)."""
    x = dist.to(freq.dtype) / cutoff
    x5 = x ** 5
    u = torch.where(x < 1, 1.0 / x + x5 * (-21.0 + x * (35.0 - 15.0 * x)), torch.zeros_like(x))
    return F.silu(F.linear(u.unsqueeze(1) * torch.sin(freq * x.unsqueeze(1)), w, b))


def local_gate(P, Q, b1, b2, i, j):
    """m_ji = SiLU(z_ji), m_nb = SiLU(z_kj) * lin_rbf(rbf) from node-side P [n, 4d] and edge-side Q [m, 4d]."""
    d = b1.numel()
    z1 = P[i, :d] + P[j, 2 * d:3 * d] + Q[:, :d] + b1
    z2 = P[i, d:2 * d] + P[j, 3 * d:] + Q[:, d:2 * d] + b2
    return F.silu(z1), F.silu(z2) * Q[:, 2 * d:3 * d]
