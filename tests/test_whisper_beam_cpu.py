"""CPU checks of WhisperMoP beam search (no GPU): signatures and defaults of beam_search and the new ops,
the support queries and bad-argument returns of mopk_decode_attn_rows_* / mopk_beam_*, the ValueErrors
raised before any device work, the row-table gather of ops.decode_attention_rows_torch, ops.beam_step_torch against a plain-Python
oracle of the documented step on hand-built logits (ties, -inf scores, eos, done items), and beam_search with every core routed
through its torch composition against a naive oracle that re-runs decode(enc, full ids) for every beam at every step."""
import ctypes as C
import inspect
import math

import pytest
import torch
import torch.nn.functional as F

NEG = float("-inf")


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


def _params(f):
    return {k: (v.default, v.kind) for k, v in inspect.signature(f).parameters.items() if k != "self"}


def test_signatures():
    from mop_amd import ops
    from mop_amd.nn import WhisperMoP
    e, P = inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert _params(WhisperMoP.beam_search) == dict(mel=(e, P), prompt_ids=(e, P), max_new_tokens=(e, P), num_beams=(e, P),
                                                   eos_token_id=(None, P), length_penalty=(1.0, P), graph=(False, P))
    rows = dict(q=(e, P), k_cache=(e, P), v_cache=(e, P), rows=(e, P), kv_len=(None, P), causal=(False, P))
    for f in (ops.decode_attention_rows, ops.decode_attention_rows_torch, ops.decode_attention_rows_supported):
        assert _params(f) == rows, f.__name__
    for f in (ops.beam_step, ops.beam_step_torch, ops.beam_step_supported):
        assert _params(f) == dict(logits=(e, P), state=(e, P), pos=(e, P)), f.__name__
    assert _params(ops.BeamState.__init__) == dict(prompt_ids=(e, P), num_beams=(e, P), cap=(e, P), eos_token_id=(None, P),
                                                   length_penalty=(1.0, P))
    assert _params(ops.beam_finalize) == dict(state=(e, P), n_new=(e, P))


def _rows_args(B=10, H=8, dk=64, cap=448, bf16=True, ld=448):
    from mop_amd import _lib
    a = _lib.DecodeAttnRowsArgs()
    b = a.base
    b.B, b.H, b.Tq, b.dk, b.cap, b.Nk, b.causal = B, H, 1, dk, cap, cap, 1
    b.io_dtype = _lib.MOPK_BF16 if bf16 else _lib.MOPK_F32
    for t in (b.k, b.v):
        t.sb, t.sh, t.sn = cap * H * dk, dk, H * dk
    a.rows_ld = ld
    return a


def test_rows_support_query_and_bad_arguments(lib):
    ok = lambda a: lib.mopk_decode_attn_rows_supported(C.byref(a))
    for dk in (32, 64, 128):
        for bf16 in (True, False):
            assert ok(_rows_args(dk=dk, bf16=bf16)) == 1
    assert ok(_rows_args(dk=48)) == 0 and ok(_rows_args(ld=447)) == 0
    a = _rows_args()
    a.rows = 2                                            # not int32-aligned
    assert ok(a) == 0
    ws = lambda a: lib.mopk_decode_attn_rows_workspace_bytes(C.byref(a))
    assert ws(_rows_args(B=40, H=8, cap=448)) == 40 * 8 * 4 * 1 * (64 + 2) * 4      # 448 keys in 128-key chunks
    assert ws(_rows_args(ld=10)) == 0
    fn = lib.mopk_decode_attn_rows_fwd
    assert fn(None, None) == -2
    assert fn(C.byref(_rows_args(ld=100)), None) == -1
    assert fn(C.byref(_rows_args(dk=96)), None) == -3
    assert fn(C.byref(_rows_args()), None) == -2          # valid shape, null tensors and table


def _beam_args(B=8, K=5, V=51865, T=224, bf16=True, eos=50257, Tp=4):
    from mop_amd import _lib
    a = _lib.BeamArgs()
    a.B, a.K, a.V, a.T, a.eos, a.prompt_len, a.length_penalty = B, K, V, T, eos, Tp, 1.0
    a.logits_dtype = _lib.MOPK_BF16 if bf16 else _lib.MOPK_F32
    a.logits_sb, a.logits_sk, a.hist_ld, a.rows_ld = K * V, V, T, T
    return a


def test_beam_support_query_and_bad_arguments(lib):
    ok = lambda a: lib.mopk_beam_supported(C.byref(a))
    for K in range(1, 9):
        for bf16 in (True, False):
            assert ok(_beam_args(K=K, bf16=bf16)) == 1, (K, bf16)
    assert ok(_beam_args(K=0)) == 0 and ok(_beam_args(K=9)) == 0
    assert ok(_beam_args(V=1, eos=-1)) == 0 and ok(_beam_args(V=2, eos=-1)) == 1 and ok(_beam_args(V=2, eos=2)) == 0
    assert ok(_beam_args(eos=-2)) == 0 and ok(_beam_args(eos=-1)) == 1
    assert ok(_beam_args(Tp=0)) == 0 and ok(_beam_args(Tp=224)) == 0
    a = _beam_args()
    a.hist_ld = 223
    assert ok(a) == 0
    a = _beam_args()
    a.logits_dtype = 2
    assert ok(a) == 0
    a = _beam_args()
    a.logits_sk = 0                                      # one logit row shared by an item's beams
    assert ok(a) == 1
    a = _beam_args()
    a.logits = 2                                         # not fp32-aligned
    assert ok(_beam_args(bf16=False)) == 1 and ok(a) == 1
    a = _beam_args(bf16=False)
    a.logits = 2
    assert ok(a) == 0
    a = _beam_args()
    a.length_penalty = float("nan")
    assert ok(a) == 0
    ws = lambda a: lib.mopk_beam_workspace_bytes(C.byref(a))
    # B * K = 40 rows: 13 slices each (512 / 40), (m, l) and 10 candidates of (logit, index) per slice
    assert ws(_beam_args()) == 40 * 13 * (2 + 20) * 4
    # B = 1, K = 5: the slices grow to fill the GPU, up to one 16-byte vector per thread (51865 / 8 / 128 = 50)
    assert ws(_beam_args(B=1)) == 5 * 50 * (2 + 20) * 4
    assert ws(_beam_args(K=9)) == 0
    fn = lib.mopk_beam_step
    assert fn(None, None) == -2
    assert fn(C.byref(_beam_args(K=9)), None) == -3
    assert fn(C.byref(_beam_args(B=0)), None) == -1
    assert fn(C.byref(_beam_args()), None) == -2         # valid shape, null tensors


def _tiny_model(**kw):
    from mop_amd.nn import WhisperConfig, WhisperMoP
    cfg = dict(n_mels=10, n_audio_ctx=40, vocab_size=100, n_text_ctx=64, n_embd=32, n_head=2, n_layer_enc=1, n_layer_dec=2,
               n_views=3, n_kernels=2, kernel_size=3)
    cfg.update(kw)
    torch.manual_seed(0)
    return WhisperMoP(WhisperConfig(**cfg)).eval()


def test_value_errors_before_device_work():
    m = _tiny_model()
    mel, ids = torch.randn(2, 40, 10), torch.zeros(2, 4, dtype=torch.long)
    for nb in (0, 9, -1):
        with pytest.raises(ValueError, match="num_beams"):
            m.beam_search(mel, ids, 5, nb)
    with pytest.raises(ValueError, match="prompt"):
        m.beam_search(mel, ids[:, :0], 5, 2)
    with pytest.raises(ValueError, match="n_text_ctx"):
        m.beam_search(mel, ids, 61, 2)                   # 4 + 61 > 64; a CPU encode would raise RuntimeError instead
    with pytest.raises(ValueError, match="vocab_size"):
        _tiny_model(vocab_size=1).beam_search(mel, ids, 5, 2)


def test_op_shape_errors():
    from mop_amd import ops
    q, k = torch.randn(2, 1, 4, 32), torch.randn(2, 10, 4, 32)
    rows = torch.zeros(2, 10, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.decode_attention_rows(q, k, torch.randn(2, 11, 4, 32), rows)
    with pytest.raises(ValueError):
        ops.decode_attention_rows(q, k, k, rows[:, :9])
    with pytest.raises(ValueError):
        ops.decode_attention_rows(q, k, k, rows[:1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.decode_attention_rows(q, k, k, rows)
    st = ops.BeamState(torch.zeros(2, 3, dtype=torch.long), 2, 8)
    pos = torch.tensor([3], dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.beam_step(torch.randn(3, 10), st, pos)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.beam_step(torch.randn(4, 10), st, pos)


def test_rows_torch_composition_gathers_the_table():
    from mop_amd import ops
    torch.manual_seed(2)
    B, cap, H, dk = 4, 20, 2, 16
    k, v = torch.randn(B, cap, H, dk), torch.randn(B, cap, H, dk)
    q = torch.randn(B, 1, H, dk)
    rows = torch.randint(0, B, (B, cap + 3), dtype=torch.int32)
    L = torch.tensor([13], dtype=torch.int32)
    got = ops.decode_attention_rows_torch(q, k, v, rows, kv_len=L, causal=True)
    for b in range(B):
        kb = torch.stack([k[int(rows[b, j]), j] for j in range(cap)])
        vb = torch.stack([v[int(rows[b, j]), j] for j in range(cap)])
        s = torch.einsum("hd,jhd->hj", q[b, 0].double(), kb[:13].double()) / dk ** 0.5
        ref = torch.einsum("hj,jhd->hd", s.softmax(-1), vb[:13].double()).reshape(-1)
        assert (got[b, 0].double() - ref).abs().max() < 1e-5
    ident = torch.arange(B, dtype=torch.int32).unsqueeze(1).repeat(1, cap)
    assert torch.equal(ops.decode_attention_rows_torch(q, k, v, ident, kv_len=L, causal=True),
                       ops.decode_attention_torch(q, k, v, kv_len=L, causal=True))


# ---- plain-Python oracle of one step (the documented semantics, over all K * V candidates) ----
def _oracle_step(logits, scores, hist, rows, fin, done, pos, K, Tp, eos, lp):
    """logits: (B*K, V) fp32 tensor; scores: list of floats; hist / rows: lists of lists; fin: per item list of (score, tokens);
    done: list of bools.  Returns the new (scores, hist, rows, fin, done, parents, next_ids) as Python values."""
    B, V = len(done), logits.shape[1]
    lse = torch.logsumexp(logits, dim=-1)
    scores, hist, rows = list(scores), [list(h) for h in hist], [list(r) for r in rows]
    fin, done = [list(f) for f in fin], list(done)
    parents, nxt = [None] * (B * K), [None] * (B * K)
    for b in range(B):
        if done[b]:
            continue
        cands = []
        for k in range(K):
            s0 = torch.tensor(scores[b * K + k], dtype=torch.float32)
            for v in range(V):
                x = logits[b * K + k, v]
                s = NEG if (x == NEG or s0 == NEG) else float(s0 + (x - lse[b * K + k]))
                cands.append((s, k * V + v))
        cands.sort(key=lambda c: (-c[0], c[1]))
        live = []
        for s, flat in cands[:2 * K]:
            if len(live) == K:
                break
            k, v = divmod(flat, V)
            if v == eos and math.isfinite(s):
                if len(fin[b]) < K:
                    norm = float(torch.tensor(float(pos - Tp + 1)).pow(lp))
                    fin[b].append((float(torch.tensor(s) / norm), hist[b * K + k][:pos] + [eos]))
            else:
                live.append((s, k, v))
        old_h, old_r = [hist[b * K + k][:] for k in range(K)], [rows[b * K + k][:] for k in range(K)]
        for i, (s, k, v) in enumerate(live):
            r = b * K + i
            scores[r], parents[r], nxt[r] = s, k, v
            hist[r][:pos] = old_h[k][:pos]
            hist[r][pos] = v
            rows[r][:pos] = old_r[k][:pos]
            rows[r][pos] = r
        done[b] = len(fin[b]) >= K
    return scores, hist, rows, fin, done, parents, nxt


def _state_py(st):
    B, K, T = st.B, st.K, st.T
    fin = [[(float(st.fin_scores[b, j]), st.fin_tokens[b, j].tolist()) for j in range(int(st.fin_count[b]))] for b in range(B)]
    return st.scores.tolist(), st.hist.tolist(), st.rows.tolist(), fin, [bool(d) for d in st.done]


def _check_step(st, logits, pos, eos, lp):
    from mop_amd import ops
    K, Tp = st.K, st.prompt_len
    x = logits.float() if logits.shape[0] == st.B * K else logits.float().repeat_interleave(K, 0)
    sc, hi, ro, fi, dn = _state_py(st)
    want = _oracle_step(x, sc, hi, ro, fi, dn, pos, K, Tp, eos, lp)
    par_old, nxt_old = st.parents.tolist(), st.next_ids.view(-1).tolist()
    ops.beam_step_torch(logits, st, torch.tensor([pos], dtype=torch.int32))
    sc2, hi2, ro2, fi2, dn2 = _state_py(st)
    w_sc, w_hi, w_ro, w_fi, w_dn, w_par, w_nxt = want
    assert dn2 == w_dn
    for b in range(st.B):
        assert len(fi2[b]) == len(w_fi[b]), b
        for (s1, t1), (s2, t2) in zip(fi2[b], w_fi[b]):
            assert s1 == pytest.approx(s2, rel=1e-6) and t1[:len(t2)] == t2 and all(t == eos for t in t1[len(t2):])
        for k in range(K):
            r = b * K + k
            assert hi2[r][:pos + 1] == w_hi[r][:pos + 1] and ro2[r][:pos + 1] == w_ro[r][:pos + 1], (b, k)
            if w_par[r] is None:                                  # done before the step: untouched
                assert st.parents[r] == par_old[r] and st.next_ids[r, 0] == nxt_old[r]
                assert sc2[r] == sc[r] or (math.isinf(sc2[r]) and math.isinf(sc[r]))
                continue
            assert int(st.parents[r]) == w_par[r] and int(st.next_ids[r, 0]) == w_nxt[r], (b, k)
            assert sc2[r] == pytest.approx(w_sc[r], rel=1e-6) or (sc2[r] == NEG and w_sc[r] == NEG)


def test_beam_step_torch_matches_the_python_oracle():
    from mop_amd import ops
    torch.manual_seed(3)
    B, K, V, Tp, T, eos = 3, 3, 7, 2, 9, 5
    st = ops.BeamState(torch.tensor([[1, 2], [3, 4], [0, 6]]), K, T, eos_token_id=eos, length_penalty=0.7)
    # first step: one shared row per item; item 0 has ties (equal logits, the smaller index first), item 2 makes eos the best
    lg = torch.randn(B, V)
    lg[0, 1] = lg[0, 3] = lg[0, 6] = 2.5
    lg[1, 2] = NEG
    lg[2, eos] = 9.0
    _check_step(st, lg, Tp, eos, 0.7)
    assert int(st.fin_count[2]) == 1 and float(st.fin_scores[2, 0]) > -0.01     # eos finished at once, gen_len 1
    for pos in range(Tp + 1, T):
        lg = torch.randn(B * K, V) * 2
        lg[0:K, eos] += 3.0                              # item 0 finishes hypotheses mid-run
        lg[K + 1, :] = NEG                               # a beam row with no finite logit
        lg[2 * K:, eos] = torch.tensor([8.0, 7.0, 6.5])
        lg[2 * K, 0] = lg[2 * K, 4]                      # a tie across the candidate list
        _check_step(st, lg, pos, eos, 0.7)
    assert bool(st.done[2]) and bool(st.done[0])         # done items were carried through the remaining steps untouched


def test_beam_step_torch_without_eos_and_tiny_vocab():
    from mop_amd import ops
    torch.manual_seed(4)
    for K, V in ((8, 2), (4, 3), (1, 2), (5, 16)):
        st = ops.BeamState(torch.zeros(2, 1, dtype=torch.long), K, 6)
        _check_step(st, torch.randn(2, V), 1, None, 1.0)
        for pos in range(2, 6):
            _check_step(st, torch.randn(2 * K, V), pos, None, 1.0)


def test_beam_step_leaves_an_out_of_range_position_alone():
    from mop_amd import ops
    st = ops.BeamState(torch.zeros(1, 2, dtype=torch.long), 2, 5, eos_token_id=1)
    before = [t.clone() for t in (st.scores, st.hist, st.rows, st.fin_tokens, st.fin_count, st.done)]
    for pos in (1, 5):
        ops.beam_step_torch(torch.randn(1, 4), st, torch.tensor([pos], dtype=torch.int32))
    after = (st.scores, st.hist, st.rows, st.fin_tokens, st.fin_count, st.done)
    assert all(torch.equal(a, b) for a, b in zip(before, after))


@pytest.fixture
def torch_cores(monkeypatch):
    """route every core through its torch composition so the module logic runs on the CPU"""
    from mop_amd import ops

    def sdpa(q, k=None, v=None, attn_mask=None, bias=None, causal=False, dropout_p=0.0, seed=None):
        y = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), attn_mask=bias, is_causal=causal)
        return y.transpose(1, 2).reshape(q.shape[0], q.shape[1], -1)

    monkeypatch.setattr(ops, "sdpa_core", sdpa)
    monkeypatch.setattr(ops, "decode_attention", lambda q, k, v, kv_len=None, nk=None, causal=False:
                        ops.decode_attention_torch(q, k, v, kv_len, nk, causal))
    monkeypatch.setattr(ops, "decode_attention_rows", ops.decode_attention_rows_torch)
    monkeypatch.setattr(ops, "beam_step", ops.beam_step_torch)


@torch.no_grad()
def naive_beam_search(m, mel, prompt, n_new, K, eos=None, lp=1.0):
    """the documented search, re-running decode(enc, full ids) for every beam at every step -> (tokens, scores, min margin at the
    K-th / 2K-th rank boundaries)"""
    enc, _ = m.encode(mel)
    B, Tp = prompt.shape
    out, outs, margin = [], [], float("inf")
    for b in range(B):
        beams = [(prompt[b].tolist(), 0.0 if k == 0 else NEG) for k in range(K)]
        fin, done = [], False
        for t in range(n_new):
            ids = torch.tensor([s for s, _ in beams], dtype=prompt.dtype, device=prompt.device)
            lg = m.decode(enc[b:b + 1].expand(K, -1, -1), ids)[:, -1].float()
            lse = torch.logsumexp(lg, dim=-1, keepdim=True)
            s0 = torch.tensor([s for _, s in beams], dtype=torch.float32, device=lg.device).unsqueeze(1)
            sc = torch.where((lg == NEG) | (s0 == NEG), torch.tensor(NEG, device=lg.device), s0 + (lg - lse)).cpu()
            V = lg.shape[1]
            cands = sorted(((float(sc[k, v]), k * V + v) for k in range(K) for v in range(V)), key=lambda c: (-c[0], c[1]))
            fs = [c[0] for c in cands if math.isfinite(c[0])]
            for r in (K, 2 * K):
                if len(fs) > r:
                    margin = min(margin, fs[r - 1] - fs[r])
            new = []
            for s, flat in cands[:2 * K]:
                if len(new) == K:
                    break
                k, v = divmod(flat, V)
                if eos is not None and v == eos and math.isfinite(s):
                    if len(fin) < K:
                        fin.append((float(torch.tensor(s) / torch.tensor(float(t + 1)).pow(lp)), beams[k][0] + [v]))
                else:
                    new.append((beams[k][0] + [v], s))
            beams = new
            if len(fin) >= K:
                done = True
                break
        if not done:
            for seq, s in beams[:K - len(fin)]:
                fin.append((float(torch.tensor(s) / torch.tensor(float(n_new)) ** lp), seq))
        best = max(range(len(fin)), key=lambda i: (fin[i][0], -i))
        seq = fin[best][1] + [eos] * (Tp + n_new - len(fin[best][1]))
        out.append(seq)
        outs.append(fin[best][0])
    return torch.tensor(out, dtype=prompt.dtype), torch.tensor(outs), margin


@pytest.mark.parametrize("K", [1, 3, 5])
def test_beam_search_matches_the_naive_oracle_with_torch_cores(torch_cores, K):
    m = _tiny_model()
    with torch.no_grad():
        m.dec_ln_f.weight.mul_(8.0)                      # spread the logits: clear rank margins
    torch.manual_seed(11)
    mel = torch.randn(2, 40, 10)
    prompt = torch.randint(0, 100, (2, 3))
    tok0, sc0 = m.beam_search(mel, prompt, 10, K)
    ref0, rs0, margin = naive_beam_search(m, mel, prompt, 10, K)
    assert margin > 1e-4
    assert torch.equal(tok0, ref0) and torch.allclose(sc0, rs0, rtol=1e-5)
    eos = int(tok0[0, 3 + 3])                            # the best beam of item 0 emits it as its 4th token
    tok, sc = m.beam_search(mel, prompt, 10, K, eos_token_id=eos, length_penalty=0.8)
    ref, rs, margin = naive_beam_search(m, mel, prompt, 10, K, eos=eos, lp=0.8)
    assert margin > 1e-4
    assert torch.equal(tok, ref) and torch.allclose(sc, rs, rtol=1e-5)
    hit = (tok[:, 3:] == eos).float().argmax(1)
    assert ((tok[:, 3:] == eos).any(1) & (hit < 9)).any()    # a hypothesis ended mid-run
    assert tok.dtype == prompt.dtype and sc.dtype == torch.float32 and tok.shape == (2, 13)


def test_one_beam_is_greedy_with_torch_cores(torch_cores):
    m = _tiny_model()
    mel, prompt = torch.randn(2, 40, 10), torch.randint(0, 100, (2, 3))
    greedy = m.generate(mel, prompt, 12)
    tok, _ = m.beam_search(mel, prompt, 12, 1)
    assert torch.equal(tok, greedy)
    eos = int(greedy[0, 6])
    assert torch.equal(m.beam_search(mel, prompt, 12, 1, eos_token_id=eos)[0], m.generate(mel, prompt, 12, eos_token_id=eos))
