"""What every entry point refuses before it launches anything, pinned op by op: which pointer fields the support query looks at and
at which alignment, and the error code of a missing pointer.  No device is needed: no call here passes every check.

One row per export whose `_supported` query takes only its args struct.  A row holds a minimal fill the query accepts (fake,
never dereferenced, 256-byte-aligned addresses in every pointer field), the alignment mask of EVERY pointer field (0: not looked
at), and one launch entry with the pointer it needs.  A row may add: `absent`, pointer fields the query wants null (setting one
flips it to 0); `views`, views read with 16-byte vectors and the element count `al` their sb / sh / sn must divide by (half of it
flips the query, `al` itself does not); `ext`, a real MopkEdgewiseExt the check reads through.  An array of pointers counts with
its first ARRAY_ELEMS entries.  The rows were read off the checks as they stood before the host launch header
(csrc/host_launch.h) replaced the open-coded tests, and passed on that tree unchanged.
"""
import ctypes as C

import pytest

BAD_ARG = -2


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


ARRAY_ELEMS = 2          # entries of a pointer array that the rows fill and test (MopkMoeArgs: E = 2 experts)


def _pointer_fields(cls, prefix=""):
    out = []
    for name, tp in cls._fields_:
        if tp is C.c_void_p:
            out.append(prefix + name)
        elif isinstance(tp, type) and issubclass(tp, C.Array) and tp._type_ is C.c_void_p:
            out += [f"{prefix}{name}[{i}]" for i in range(ARRAY_ELEMS)]
        elif isinstance(tp, type) and issubclass(tp, C.Structure):
            out += _pointer_fields(tp, prefix + name + ".")
    return out


def _set(a, path, value):
    *head, leaf = path.split(".")
    for h in head:
        a = getattr(a, h)
    if leaf.endswith("]"):
        name, i = leaf[:-1].split("[")
        getattr(a, name)[int(i)] = value
    else:
        setattr(a, leaf, value)


F32 = 0
DA = dict(B=1, H=1, Tq=1, dk=32, cap=64, Nk=64, io_dtype=F32, causal=0,
          **{f"{t}.{s}": v for t in "qkvy" for s, v in (("sb", 2048), ("sh", 2048), ("sn", 32))})
DA_MASKS = {"q.ptr": 0, "k.ptr": 15, "v.ptr": 15, "y.ptr": 0, "kv_len": 3, "workspace": 15}
SP = dict(R=1, n=1, V=8, logits_dtype=F32, top_k=0, greedy=0, inv_temp=1.0, top_p=1.0, logits_sb=8, logits_sk=8)
SP_MASKS = {"logits": 3, "pos": 0, "tokens": 0, "logprobs": 0, "workspace": 0}


def _base(d):
    return {"base." + k: v for k, v in d.items()}


def _strides(views, d):
    """contiguous (1, 1, 8 or 32, d) views: sb = sh = 32 d, sn = d"""
    return {f"{v}.{s}": n for v in views for s, n in (("sb", 32 * d), ("sh", 32 * d), ("sn", d))}


SD = dict(B=1, H=1, N=8, dk=32, io_dtype=F32, precision=1, path=0, causal=0, Nk=0, **_strides(("q", "k", "v", "y"), 32))
SD_MASKS = {"q.ptr": 15, "k.ptr": 15, "v.ptr": 15, "y.ptr": 15, "mask": 0, "bias": 0, "saved": 0, "workspace": 0,
            "dy.ptr": 0, "dq.ptr": 0, "dk_.ptr": 0, "dv.ptr": 0}


# (struct, support query, scalar fill, {pointer field: mask}, launch entry, pointer that entry needs)
ROWS = [
    ("AlignCostArgs", "mopk_alignment_cost_supported", dict(B=1, S=1, N=4, M=4, width=1, cost_ld=4),
     {"probs": 3, "n_tokens": 3, "n_frames": 3, "cost": 3}, "mopk_alignment_cost", "probs"),
    ("DtwArgs", "mopk_dtw_align_supported", dict(B=1, N=4, M=4, row0=0, cost_ld=4),
     {"cost": 3, "n_rows": 3, "n_cols": 3, "starts": 3, "ends": 3, "workspace": 0}, "mopk_dtw_align", "workspace"),
    ("LogMelArgs", "mopk_log_mel_supported", dict(B=1, L=1600, n_fft=400, hop=160, n_mels=80, audio_dtype=F32, out_dtype=F32, audio_ld=1600),
     {"audio": 3, "lens": 3, "filters": 3, "bands": 3, "twiddle": 7, "window": 3, "out": 3, "workspace": 3}, "mopk_log_mel", "twiddle"),
    ("ResampleArgs", "mopk_resample_supported",
     dict(B=1, C=1, L=64, Lout=64, o=1, n=1, w=4, S=9, table_ld=16, audio_dtype=F32, out_dtype=F32, audio_sb=64, audio_sc=64, audio_sl=1),
     {"audio": 3, "lens": 3, "table": 3, "first": 3, "out": 3, "out_lens": 3}, "mopk_resample", "first"),
    ("TimestampSegmentsArgs", "mopk_timestamp_segments_supported", dict(R=1, T=8, T0=1, tb=100, eos=50, f=2, tokens_ld=8),
     {"tokens": 3, "window": 3, "starts": 3, "ends": 3, "tok_begin": 3, "tok_end": 3, "n_segments": 3, "advance": 3},
     "mopk_timestamp_segments", "advance"),
    ("PromptHistoryArgs", "mopk_prompt_history_update_supported", dict(A=1, B=1, n=8, T=8, T0=1, tokens_ld=8),
     {"hist": 3, "hist_len": 3, "tokens": 3, "n_take": 3, "item": 3, "mode": 3}, "mopk_prompt_history_update", "mode"),
    ("WindowPromptsArgs", "mopk_window_prompts_supported", dict(A=1, B=1, n=8, width=8, Ts=4, prev=0, out_i64=0, sot_i64=1, sot_ld=0),
     {"hist": 3, "hist_len": 3, "item": 3, "sot": 7, "ids": 3, "kv_start": 3}, "mopk_window_prompts", "sot"),
    ("AlignmentRowsArgs", "mopk_alignment_rows_supported", dict(R=1, T=8, T0=1, Tp=4, nots=0, eos=50, out_i64=1, sot_i64=0, tokens_ld=8, sot_ld=0),
     {"tokens": 3, "n_take": 3, "sot": 3, "ids": 7, "n_tokens": 3, "col": 3}, "mopk_alignment_rows", "col"),
    ("WordSpansArgs", "mopk_word_spans_supported", dict(R=1, N=8, V=100, median_cap=-1, tokens_ld=8, times_ld=9, probs_ld=8),
     {"tokens": 3, "times": 3, "probs": 3, "n_text": 3, "table": 0, "starts": 3, "ends": 3, "out_probs": 3, "tok_begin": 3,
      "tok_end": 3, "n_words": 3}, "mopk_word_spans", "table"),
    ("TokenLogprobArgs", "mopk_token_logprob_supported", dict(R=1, V=8, dtype=F32, token=1, logits_ld=8),
     {"logits": 3, "tokens": 3, "out": 3}, "mopk_token_logprob", "out"),
    ("GreedyPickArgs", "mopk_greedy_pick_supported", dict(R=1, V=8, dtype=F32, eos=1, hist_cap=4, hist_ld=4, logits_ld=8),
     {"logits": 3, "pos": 3, "next_ids": 3, "done": 3, "sum_logprobs": 3, "n_tokens": 3, "hist": 3}, "mopk_greedy_pick", "done"),
    ("LanguageProbsArgs", "mopk_language_probs_supported", dict(R=1, V=8, dtype=F32, n=2, logits_ld=8, probs_ld=2),
     {"logits": 3, "ids": 3, "probs": 3, "tokens": 3}, "mopk_language_probs", "ids"),
    ("LogitRulesArgs", "mopk_logit_rules_supported", dict(R=1, V=8, dtype=F32, T=4, T0=1, tb=-1, eos=0, max_initial=-1, logits_ld=8, out_ld=8, hist_ld=4),
     {"logits": 3, "out": 3, "hist": 3, "pos": 3, "mask": 0}, "mopk_logit_rules", "mask"),
    ("RepeatRulesArgs", "mopk_repeat_rules_supported",
     dict(R=1, V=8, dtype=F32, T=4, T0=1, ngram=0, penalty=1.5, inv_penalty=0.5, logits_ld=8, out_ld=8, hist_ld=4),
     {"logits": 3, "out": 3, "hist": 3, "pos": 3, "exempt": 0}, "mopk_repeat_rules", "exempt"),
    ("SampleArgs", "mopk_sample_supported", SP, SP_MASKS, "mopk_sample_step", "logprobs"),
    ("SampleRaggedArgs", "mopk_sample_ragged_supported", _base(SP), {**_base(SP_MASKS), "pos_off": 3}, "mopk_sample_ragged_step", "base.tokens"),
    ("BeamArgs", "mopk_beam_supported",
     dict(B=1, K=2, V=8, T=8, logits_dtype=F32, eos=1, prompt_len=1, length_penalty=1.0, logits_sb=16, logits_sk=8, hist_ld=8, rows_ld=8),
     {"logits": 3, "pos": 0, "scores": 0, "next_ids": 0, "parents": 0, "hist": 0, "rows": 0, "fin_tokens": 0, "fin_scores": 0,
      "fin_count": 0, "done": 0, "workspace": 15}, "mopk_beam_step", "fin_count"),
    ("TokenGateArgs", "mopk_token_gate_supported", dict(B=1, T=4, D=8, x_dtype=F32, a_dtype=F32, o_dtype=F32, x_sb=32, x_st=8, a_sb=32, a_st=8),
     {"x": 15, "a": 15, "u": 15, "out": 15, "gate": 0, "dout": 15, "dr": 15, "du": 15, "workspace": 15}, "mopk_token_gate_fwd", "gate"),
    ("MelGateArgs", "mopk_mel_gate_supported", dict(B=1, T=4, F=8, L=1, k=3, mel_dtype=F32, mel_sb=32, mel_st=8),
     {"mel": 3, "W": 3, "lens": 3, "gates": 3, "dgates": 3, "dW": 3, "workspace": 3}, "mopk_mel_gate_fwd", "gates"),
    ("GatedResidualArgs", "mopk_gated_residual_supported",
     dict(B=1, T=4, D=8, x_dtype=F32, a_dtype=F32, o_dtype=F32, x_sb=32, x_st=8, a_sb=32, a_st=8, gate_sb=4),
     {"x": 15, "a": 15, "gate": 3, "out": 15, "dout": 15, "dr": 15, "dgate": 3}, "mopk_gated_residual_bwd", "dgate"),
    ("DecodeAttnArgs", "mopk_decode_attn_supported", DA, DA_MASKS, "mopk_decode_attn_fwd", "y.ptr", {"views": {"k": 4, "v": 4}}),
    ("DecodeAttnRowsArgs", "mopk_decode_attn_rows_supported", {**_base(DA), "rows_ld": 64}, {**_base(DA_MASKS), "rows": 3},
     "mopk_decode_attn_rows_fwd", "rows", {"views": {"base.k": 4, "base.v": 4}}),
    ("DecodeAttnRaggedArgs", "mopk_decode_attn_ragged_supported", {**_base(DA), "rows_ld": 64}, {**_base(DA_MASKS), "rows": 3, "kv_start": 3},
     "mopk_decode_attn_ragged_fwd", "base.q.ptr", {"views": {"base.k": 4, "base.v": 4}}),
    # per-row key lengths take the place of the one kv_len, which must be absent
    ("DecodeAttnLensArgs", "mopk_decode_attn_lens_supported", _base(DA),
     {**{k: m for k, m in _base(DA_MASKS).items() if k != "base.kv_len"}, "kv_lens": 3},
     "mopk_decode_attn_lens_fwd", "base.y.ptr", {"absent": ["base.kv_len"], "views": {"base.k": 4, "base.v": 4}}),
    # ---- the attention cores: fp32 tensors (al = 4 elements per 16-byte vector), bf16 arithmetic
    ("SdpaArgs", "mopk_sdpa_fused_supported", SD, SD_MASKS, "mopk_sdpa_fwd", "saved", {"views": dict.fromkeys(("q", "k", "v", "y"), 4)}),
    ("SdpaLensArgs", "mopk_sdpa_lens_supported", _base(SD),
     {**{k: m for k, m in _base(SD_MASKS).items() if k not in ("base.mask", "base.bias")}, "q_lens": 3, "kv_lens": 3},
     "mopk_sdpa_lens_fwd", "base.workspace",
     {"absent": ["base.mask", "base.bias"], "views": dict.fromkeys(("base.q", "base.k", "base.v", "base.y"), 4)}),
    ("DualPathArgs", "mopk_dualpath_fused_supported",
     dict(B=1, H=1, N=8, dk=32, hops=2, io_dtype=F32, precision=1, path=0, causal=0, g_chain=0.0,
          **_strides(("q1", "k1", "v1", "q2", "k2", "v2", "y"), 32)),
     {**{f"{v}.ptr": 15 for v in ("q1", "k1", "v1", "q2", "k2", "v2", "y")}, "mask": 0, "chain_logit": 0, "saved": 0, "workspace": 0,
      **{f"{v}.ptr": 0 for v in ("dy", "dq1", "dk1", "dv1", "dq2", "dk2", "dv2")}, "dlogit_part": 0},
     "mopk_dualpath_fwd", "chain_logit", {"views": dict.fromkeys(("q1", "k1", "v1", "q2", "k2", "v2", "y"), 4)}),
    ("QuartetArgs", "mopk_quartet_fused_supported",
     dict(B=1, H=1, T=8, dh=32, io_dtype=F32, precision=1, path=0, use_quartet=1, **_strides(("q", "k", "v", "y", "q2", "k2"), 32)),
     {**{f"{v}.ptr": 15 for v in ("q", "k", "v", "y", "q2", "k2")}, "mixture": 0, "quartet_scale": 0, "add_mask": 0, "saved": 0,
      "workspace": 0, **{f"{v}.ptr": 0 for v in ("dy", "dq", "dk_", "dv", "dq2", "dk2")}, "dmixture_part": 0, "dqscale_part": 0},
     "mopk_quartet_fwd", "mixture", {"absent": ["attn"], "views": dict.fromkeys(("q", "k", "v", "y", "q2", "k2"), 4)}),
    # the dense gate head on the fused Edgewise kernels: the query reads W1 / b1 / W2 / b2 through `ext`; no attention mask
    ("EdgewiseArgs", "mopk_edgewise_fused_supported",
     dict(B=1, H=1, N=32, dk=16, V=2, r=1, io_dtype=F32, precision=1, path=2, save_for_backward=1,
          **_strides(("q", "k", "v0", "vL", "y"), 16)),
     {**{f"{v}.ptr": 15 for v in ("q", "k", "v0", "vL", "y")},
      **dict.fromkeys(("sqk", "vs0", "vsL", "Wr", "br", "Wc", "bc", "chain_logit", "saved", "workspace", "dy.ptr", "dq.ptr", "dk_.ptr",
                       "dv0.ptr", "dvL.ptr", "dsqk_part", "dvs0_part", "dvsL_part", "dWr", "dbr", "dWc", "dbc", "dlogit_part"), 0)},
     "mopk_edgewise_fwd", "sqk",
     {"absent": ["mask"], "views": dict.fromkeys(("q", "k", "v0", "vL", "y"), 4),
      "ext": dict(gate_mode=1, W1=0x200000, b1=0x200100, W2=0x200200, b2=0x200300),
      "ext_needs": dict(W1=0x200000, b1=0x200100, W2=0x200200, b2=0x200300)}),
    # pointers are looked at when present; every expert's weight pointers count (ARRAY_ELEMS = E of them here)
    ("MoeArgs", "mopk_moe_supported", dict(M=8, D=8, F=8, E=ARRAY_ELEMS, precision=1, x_dtype=F32, w_dtype=F32, gate_dtype=F32, o_dtype=F32),
     {"x": 15, "gate_w": 0, "gate_b": 0, "residual": 15, "y": 15, "u": 15, "h": 15, "route": 15, "dy": 15, "dx": 15, "workspace": 15,
      **{f"{w}[{e}]": 15 for w in ("w1", "w2", "dw1", "dw2") for e in range(ARRAY_ELEMS)}}, "mopk_moe_route", "route"),
]


def _opts(row):
    return row[6] if len(row) > 6 else {}


def _filled(row):
    """-> the struct, the address of every pointer field, the objects that must outlive the calls"""
    from mop_amd import _lib
    struct, _, fill, masks = row[:4]
    absent = _opts(row).get("absent", ())
    cls = getattr(_lib, struct)
    assert sorted(_pointer_fields(cls)) == sorted([*masks, *absent]), f"{struct}: the row must name every pointer field"
    a = cls()
    for k, v in fill.items():
        _set(a, k, v)
    addr = {}
    for i, f in enumerate(_pointer_fields(cls)):
        addr[f] = 0x100000 + 256 * i
        if f not in absent:
            _set(a, f, addr[f])
    keep = []
    if "ext" in _opts(row):                                   # a real nested struct: the check reads through the pointer
        x = _lib.EdgewiseExt()
        for k, v in _opts(row)["ext"].items():
            setattr(x, k, v)
        a.ext = C.pointer(x)
        keep.append(x)
    return a, addr, keep


@pytest.mark.parametrize("row", ROWS, ids=[r[1] for r in ROWS])
def test_query_accepts_the_fill_and_looks_at_each_pointer_at_its_mask(lib, row):
    a, addr, keep = _filled(row)
    query = getattr(lib, row[1])
    assert query(C.byref(a)) == 1
    for f, mask in row[3].items():
        # half the alignment breaks it, the alignment itself does not; a field the query does not look at takes any address
        for off, want in (((mask + 1) // 2, 0), (mask + 1, 1)) if mask else ((1, 1),):
            _set(a, f, addr[f] + off)
            assert query(C.byref(a)) == want, f"{row[1]}: {f} at +{off} (mask {mask})"
        _set(a, f, addr[f])
    for f in _opts(row).get("absent", ()):
        _set(a, f, addr[f])
        assert query(C.byref(a)) == 0, f"{row[1]}: {f} present"
        _set(a, f, None)
    for view, al in _opts(row).get("views", {}).items():
        for s in ("sb", "sh", "sn"):
            base = row[2][f"{view}.{s}"]
            for off, want in ((al // 2, 0), (al, 1)):
                _set(a, f"{view}.{s}", base + off)
                assert query(C.byref(a)) == want, f"{row[1]}: {view}.{s} + {off} (al {al})"
            _set(a, f"{view}.{s}", base)
    for k, v in _opts(row).get("ext_needs", {}).items():     # a pointer of the nested struct that the query requires
        x = keep[0]
        setattr(x, k, None)
        assert query(C.byref(a)) == 0, f"{row[1]}: ext.{k} missing"
        setattr(x, k, v)
    assert query(C.byref(a)) == 1


@pytest.mark.parametrize("row", ROWS, ids=[r[4] for r in ROWS])
def test_entry_refuses_a_missing_pointer(lib, row):
    a, _, keep = _filled(row)
    _set(a, row[5], None)
    assert getattr(lib, row[4])(C.byref(a), None) == BAD_ARG
