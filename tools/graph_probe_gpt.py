"""test helper (GPU box): forward + backward of a 2-block bf16 GPT_MoP captured into HIP graphs (torch.cuda.make_graphed_callables)
and replayed; prints whether the gate ran on the fused kernels and whether two replays reproduce the eager loss and the parameter
gradients (bit for bit outside the embeddings).  Warm-up and capture follow tools/graph_probe.py (eager steps first, no warm-up of make_graphed_callables' own)."""
import copy
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from mop_amd import _lib, ops  # noqa: E402
from mop_amd.nn import GPT_MoP  # noqa: E402
from mop_amd.nn.quartet_attn_patch import TransformerConfig  # noqa: E402

torch.manual_seed(0)
cfg = TransformerConfig(n_layer=2, n_head=4, n_embd=256, block_size=128, dropout=0.0)
model = GPT_MoP(512, cfg, n_views=5, n_kernels=3).cuda().to(torch.bfloat16)


class Logits(torch.nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, idx):
        return self.m(idx)[0]


net = Logits(model)
idx = torch.randint(0, 512, (4, 128), device="cuda")
tgt = torch.randint(0, 512, (4, 128), device="cuda")
opt = torch.optim.AdamW(model.parameters(), lr=1e-3)


def step(f):
    opt.zero_grad(set_to_none=True)
    loss = F.cross_entropy(f(idx).float().view(-1, 512), tgt.view(-1))
    loss.backward()
    opt.step()


for _ in range(3):
    step(net)
torch.cuda.synchronize()
print("FUSED_GATE", ops.LAST_PATH.get("token_gate_fwd") == _lib.PATH_FUSED and ops.LAST_PATH.get("token_gate_bwd") == _lib.PATH_FUSED,
      flush=True)
try:
    g = torch.cuda.make_graphed_callables(net, (idx,), num_warmup_iters=0)
except RuntimeError as e:
    print("CAPTURE_UNSUPPORTED", repr(e)[:300], flush=True)
    sys.exit(0)
print("captured", flush=True)
sd = copy.deepcopy(model.state_dict())


def one(f):
    model.load_state_dict(sd)
    model.zero_grad(set_to_none=True)
    loss = F.cross_entropy(f(idx).float().view(-1, 512), tgt.view(-1))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


le, ge = one(net)
lg, gg = one(g)
lg2, gg2 = one(g)
print("loss eager %.6f graphed %.6f" % (float(le), float(lg)))
# the embedding gradients (wte.weight is also the tied head's) come from torch's embedding backward, whose accumulation order over
# repeated token ids is not fixed: those two are compared to rounding, every other tensor bit for bit
emb = ("wte.weight", "wpe.weight")
print("GRAPH_IDENTICAL", set(ge) == set(gg) and all(torch.equal(ge[k], gg[k]) and torch.equal(gg[k], gg2[k]) for k in ge if k not in emb)
      and all(torch.allclose(ge[k].float(), gg[k].float(), rtol=2e-2, atol=1e-3 * float(ge[k].float().abs().max())) for k in emb)
      and bool((le - lg).abs() <= 1e-3) and bool((lg - lg2).abs() <= 1e-3))
