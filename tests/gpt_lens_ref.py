"""float64 references of the GPT line over right-padded rows: every row ALONE, padded back with zeros.

Row b of a batch with lens[b] = n real tokens must come out as the same tokens would in a batch of their own at T = n.  The
references here are built exactly that way -- `oracle.quartet.core_fwd` / `core_bwd` and the folded token-gate formula are run on
the slices [:n] of each row and know nothing about lengths -- so they share no code with the length-aware kernels or with
`ops.quartet_core_lens_torch`.
"""
import numpy as np
import torch

from oracle import quartet as Q


def _np64(t):
    return None if t is None else t.detach().double().cpu().numpy()


def quartet_rows_alone(q, k, v, q2, k2, mixture, qscale, lens, eps, use_quartet, dy):
    """q, k, v, q2, k2: (B,T,H,dh) tensors (q2 = k2 = None without the quartet term); mixture / qscale: floats; lens: B ints; dy:
    (B,T,H*dh).  Returns float64 numpy arrays: y (B,T,H*dh), P (B,H,T,T), and the gradients dq dk dv (dq2 dk2) in (B,T,H,dh), with
    dmixture / dquartet_scale summed over the rows."""
    B, T, H, dh = q.shape
    ins = {"q": _np64(q), "k": _np64(k), "v": _np64(v)}
    if use_quartet:
        ins.update(q2=_np64(q2), k2=_np64(k2))
    g = _np64(dy).reshape(B, T, H, dh)
    out = {"y": np.zeros((B, T, H * dh)), "P": np.zeros((B, H, T, T))}
    out.update({"d" + n: np.zeros((B, T, H, dh)) for n in ins})
    if use_quartet:
        out.update(dmixture=0.0, dquartet_scale=0.0)
    for b, n in enumerate(int(x) for x in lens):
        n = max(0, min(n, T))
        if n == 0:
            continue
        row = {name: np.transpose(a[b:b + 1, :n], (0, 2, 1, 3)) for name, a in ins.items()}      # (1,H,n,dh): the row alone
        y, c = Q.core_fwd(row["q"], row["k"], row["v"], row.get("q2"), row.get("k2"), mixture, qscale, eps, use_quartet)
        gr = Q.core_bwd(np.transpose(g[b:b + 1, :n], (0, 2, 1, 3)), c)
        out["y"][b, :n] = np.transpose(y, (0, 2, 1, 3)).reshape(n, H * dh)
        out["P"][b, :, :n, :n] = c["P"][0]
        for name in ins:
            out["d" + name][b, :n] = np.transpose(gr["d" + name], (0, 2, 1, 3))[0]
        if use_quartet:
            out["dmixture"] += float(gr["dmixture"])
            out["dquartet_scale"] += float(gr["dquartet_scale"])
    return out


def token_gate_rows_alone(x, a, u, lens, dout):
    """the folded gate out_t = r_t (1 + u0.r_{t-1} + u1.r_t + u2.r_{t+1}), r = x + a, on r[:n] of each row alone (zero padding at
    both ends of the row), in float64.  Returns (out (B,T,D), dr (B,T,D), du (3,D)) as float64 CPU tensors."""
    B, T, D = x.shape
    r_all = (x.detach().double() + (0 if a is None else a.detach().double())).cpu()
    g_all = dout.detach().double().cpu()
    u64 = u.detach().double().cpu().requires_grad_(True)
    out, dr, du = torch.zeros(B, T, D, dtype=torch.float64), torch.zeros(B, T, D, dtype=torch.float64), torch.zeros(3, D, dtype=torch.float64)
    for b, n in enumerate(int(v) for v in lens):
        n = max(0, min(n, T))
        if n == 0:
            continue
        r = r_all[b, :n].clone().requires_grad_(True)
        p = r @ u64.t()                                                     # (n,3)
        gate = 1 + p[:, 1]
        gate = gate + torch.cat([p.new_zeros(1), p[:-1, 0]]) + torch.cat([p[1:, 2], p.new_zeros(1)])
        o = r * gate.unsqueeze(-1)
        gr, gu = torch.autograd.grad((o * g_all[b, :n]).sum(), (r, u64))
        out[b, :n], dr[b, :n] = o.detach(), gr
        du += gu
    return out, dr, du
