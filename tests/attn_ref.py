"""float64 references and input generators shared by the attention edge-case tests (peaked logits, fully blocked rows)."""
import torch


def bf16_exact(t: torch.Tensor) -> torch.Tensor:
    """t with every value rounded to bfloat16, kept in t's dtype: the operands a bf16-MFMA kernel reads, so a float64 reference
    on them measures the kernel's arithmetic and not the input rounding"""
    return t.to(torch.bfloat16).to(t.dtype)


def logit_qk(shape_q, shape_k, sigma: float, gen: torch.Generator, device="cuda"):
    """q, k drawn from N(0, 1) and scaled by sqrt(sigma) each, so the logits q . k / sqrt(dk) have a standard deviation of about
    sigma (shapes (.., dk))"""
    s = float(sigma) ** 0.5
    q = torch.randn(*shape_q, device=device, generator=gen) * s
    k = torch.randn(*shape_k, device=device, generator=gen) * s
    return q, k


def logit_std(q: torch.Tensor, k: torch.Tensor) -> float:
    """standard deviation of the logits q . k / sqrt(dk) over every (b, h, i, j); q (B,N,H,dk), k (B,Nk,H,dk)"""
    s = torch.einsum("bihd,bjhd->bhij", q.detach().double(), k.detach().double()) / q.shape[-1] ** 0.5
    return float(s.std())


def sdpa_ref64(q, k, v, mask=None, bias=None, causal=False):
    """float64 softmax(q k^T / sqrt(dk) + bias, over the keys mask leaves open) v, differentiable in q, k, v.
    q (B,N,H,dk), k, v (B,Nk,H,dk) -> (B,N,H*dk).  mask: 0 / False = blocked; bias: additive; both broadcastable to (B,H,N,Nk).
    A row with no open key of finite logit is 0 and takes no part in the gradients: torch's SDPA convention."""
    B, N, H, dk = q.shape
    q, k, v = (t.double().transpose(1, 2) for t in (q, k, v))
    s = q @ k.transpose(-1, -2) / dk ** 0.5
    if bias is not None:
        s = s + bias.to(s.device, torch.float64)
    if mask is not None:
        s = s.masked_fill(~mask.to(s.device).bool(), float("-inf"))
    if causal:
        s = s.masked_fill(~torch.ones(N, k.shape[-2], dtype=torch.bool, device=s.device).tril(), float("-inf"))
    m = s.detach().amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    den = e.sum(-1, keepdim=True)
    p = e / torch.where(den > 0, den, torch.ones_like(den))
    return (p @ v).transpose(1, 2).reshape(B, N, H * dk)


def blocked_rows_mask(N: int, Nk: int, gen: torch.Generator, device="cuda"):
    """(N, Nk) bool keep-mask (True = open) holding every hard row at once, and the indices of the rows it blocks fully.
    Rows: 0 fully blocked; 1 open only at key 0; 2 with its whole first 64-key tile blocked (needs Nk > 64); N - 2 fully blocked
    (in the last partial query block when N % 128 is not 0); N - 1 open only at key Nk - 1 (in the last partial key tile); the rest
    with 30 % of keys blocked at random."""
    keep = torch.rand(N, Nk, device=device, generator=gen) > 0.3
    keep[:, 0] = True
    keep[0] = False
    keep[1] = False
    keep[1, 0] = True
    if Nk > 64:
        keep[2, :64] = False
        keep[2, 64] = True
    keep[N - 2] = False
    keep[N - 1] = False
    keep[N - 1, Nk - 1] = True
    return keep
