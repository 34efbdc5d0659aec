"""The C-ABI library builds for gfx950, loads, and exports every symbol include/mopk.h declares; mop_amd/_lib.py mirrors every struct
and constant of that header (the one place that compares the two)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


def _header_functions():
    src = open(os.path.join(ROOT, "include", "mopk.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mopk_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported(lib):
    from mop_amd import _lib
    names = _header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mopk.h but not exported by libmopk.so"
        assert n in _lib.SYMBOLS, f"{n} has no ctypes prototype in mop_amd/_lib.py"


def test_version_and_strerror(lib):
    assert lib.mopk_version() == 118
    assert lib.mopk_strerror(0) == b"ok"
    assert b"shape" in lib.mopk_strerror(-1)


# Field names that the per-op tests used to write out by hand, in declaration order: a field dropped from mopk.h and from _lib.py
# together would pass the comparison below, not this table.  A new struct needs no entry; test_lib_mirrors_the_header finds it.
PINNED_FIELDS = {
    "MopkDecodeAttnArgs": ["B", "H", "Tq", "dk", "cap", "Nk", "io_dtype", "causal", "q", "k", "v", "y", "kv_len", "workspace"],
    "MopkDecodeAttnRowsArgs": ["base", "rows", "rows_ld"],
    "MopkDecodeAttnRaggedArgs": ["base", "rows", "rows_ld", "kv_start"],
    "MopkDecodeAttnLensArgs": ["base", "kv_lens"],
    "MopkSdpaLensArgs": ["base", "q_lens", "kv_lens"],
    "MopkMoeArgs": ["M", "D", "F", "E", "precision", "x_dtype", "w_dtype", "gate_dtype", "o_dtype", "reserved", "x", "gate_w", "gate_b",
                    "w1", "w2", "residual", "y", "u", "h", "route", "dy", "dx", "dw1", "dw2", "workspace"],
    "MopkBeamArgs": ["B", "K", "V", "T", "logits_dtype", "eos", "prompt_len", "length_penalty", "logits", "logits_sb", "logits_sk",
                     "pos", "scores", "next_ids", "parents", "hist", "hist_ld", "rows", "rows_ld", "fin_tokens", "fin_scores",
                     "fin_count", "done", "workspace"],
    "MopkSampleArgs": ["R", "n", "V", "logits_dtype", "top_k", "greedy", "inv_temp", "top_p", "seed", "logits", "logits_sb",
                       "logits_sk", "pos", "tokens", "logprobs", "workspace"],
    "MopkSampleRaggedArgs": ["base", "pos_off"],
    "MopkTokenLogprobArgs": ["R", "V", "dtype", "token", "logits", "logits_ld", "tokens", "out"],
    "MopkGreedyPickArgs": ["R", "V", "dtype", "eos", "hist_cap", "reserved", "logits", "logits_ld", "pos", "next_ids", "done",
                           "sum_logprobs", "n_tokens", "hist", "hist_ld"],
    "MopkLanguageProbsArgs": ["R", "V", "dtype", "n", "logits", "logits_ld", "ids", "probs", "probs_ld", "tokens"],
    "MopkAlignmentRowsArgs": ["R", "T", "T0", "Tp", "nots", "eos", "out_i64", "sot_i64", "tokens", "tokens_ld", "n_take", "sot",
                              "sot_ld", "ids", "n_tokens", "col"],
    "MopkWordSpansArgs": ["R", "N", "V", "median_cap", "tokens", "tokens_ld", "times", "times_ld", "probs", "probs_ld", "n_text",
                          "table", "starts", "ends", "out_probs", "tok_begin", "tok_end", "n_words"],
}


def _constants():
    """header macro or enumerator -> its Python twin (a literal where Python keeps none).  A new mirrored constant goes here."""
    from mop_amd import _lib, ops
    return {
        "MOPK_VERSION": 118,
        "MOPK_F32": _lib.MOPK_F32, "MOPK_BF16": _lib.MOPK_BF16,
        "MOPK_PREC_FP32": _lib.PREC_FP32, "MOPK_PREC_BF16": _lib.PREC_BF16,
        "MOPK_PATH_AUTO": _lib.PATH_AUTO, "MOPK_PATH_GENERIC": _lib.PATH_GENERIC, "MOPK_PATH_FUSED": _lib.PATH_FUSED,
        "MOPK_MAX_LENS": _lib.MAX_LENS, "MOPK_DENSE_HIDDEN": _lib.DENSE_HIDDEN, "MOPK_MOE_MAX_EXPERTS": _lib.MOE_MAX_EXPERTS,
        "MOPK_LANGUAGE_MAX_N": _lib.LANGUAGE_MAX_N, "MOPK_LOG_MEL_TILE_FRAMES": _lib.LOG_MEL_TILE_FRAMES,
        "MOPK_LOG_MEL_F16": _lib.LOG_MEL_F16, "MOPK_BEAM_MAX_K": ops.BEAM_MAX_K,
        "MOPK_SAMPLE_MAX_V": 1 << 24,
        "MOPK_MEL_GATE_TILE": 32, "MOPK_MEL_GATE_LAYERS": 8, "MOPK_MEL_GATE_MAX_K": 7, "MOPK_MEL_GATE_MAX_F": 128,
    }


def test_lib_mirrors_the_header(lib, tmp_path):
    """every ctypes.Structure of mop_amd/_lib.py against its struct in include/mopk.h -- sizeof, and offsetof and sizeof of every
    field, as the C compiler sees them -- and every mirrored constant against its value there: one generated program, one gcc run"""
    from mop_amd import _lib
    mine = {"Mopk" + n: c for n, c in vars(_lib).items()
            if isinstance(c, type) and issubclass(c, C.Structure) and c.__module__ == _lib.__name__}
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mopk.h")).read(), flags=re.S)
    structs = re.findall(r"typedef\s+struct\s+(Mopk\w+)\s*\{", src)
    enums = re.findall(r"typedef\s+enum\s+(Mopk\w+)\s*\{", src)
    assert sorted(mine) == sorted(structs) and len(set(structs)) == len(structs) > 0
    assert sorted(re.findall(r"\}\s*(Mopk\w+)\s*;", src)) == sorted(structs + enums) and len(enums) == 4
    consts = _constants()
    prog = ['#include <stdio.h>', '#include "mopk.h"', 'int main(void){']
    for name, cls in mine.items():
        prog.append(f'printf("{name} %zu\\n", sizeof({name}));')
        prog += [f'printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name} *)0)->{f}));' for f, _ in cls._fields_]
    prog += [f'printf("{c} %lld\\n", (long long)({c}));' for c in consts] + ['return 0;}', '']
    (tmp_path / "abi.c").write_text("\n".join(prog))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")])
    out = subprocess.check_output([str(tmp_path / "abi")], text=True)
    got = {k: tuple(map(int, v)) for k, *v in map(str.split, out.splitlines())}       # name -> (sizeof,) | (offsetof, sizeof) | (value,)
    n_fields = 0
    for name, cls in mine.items():
        names = [f for f, _ in cls._fields_]
        assert names == PINNED_FIELDS.get(name, names), f"{name}: the fields are no longer those pinned in PINNED_FIELDS"
        bad = [f for f in names if got[f"{name}.{f}"] != (getattr(cls, f).offset, getattr(cls, f).size)]
        assert not bad, (f"{name}.{bad[0]}: (offset, size) {got[name + '.' + bad[0]]} in mopk.h, "
                         f"{(getattr(cls, bad[0]).offset, getattr(cls, bad[0]).size)} in _lib.py")
        assert got[name] == (C.sizeof(cls),), f"{name}: sizeof {got[name][0]} in mopk.h, {C.sizeof(cls)} in _lib.py"
        n_fields += len(names)
    assert len(got) == len(structs) + n_fields + len(consts)          # nothing printed twice, nothing lost
    assert set(PINNED_FIELDS) <= set(mine)
    for c, twin in consts.items():
        assert got[c] == (twin,), f"{c}: {got[c][0]} in mopk.h, {twin} in Python"
    assert lib.mopk_version() == consts["MOPK_VERSION"]


def test_size_queries_need_no_gpu(lib):
    from mop_amd import _lib
    a = _lib.EdgewiseArgs()
    a.B, a.H, a.N, a.dk, a.V, a.r = 2, 6, 197, 64, 5, 4
    s = lib.mopk_edgewise_saved_bytes(C.byref(a))
    w = lib.mopk_edgewise_workspace_bytes(C.byref(a))
    assert s > 0 and w > 0
    a.N = 0
    assert lib.mopk_edgewise_saved_bytes(C.byref(a)) == 0


def test_lens_means_support_query_needs_no_gpu(lib):
    """mopk_lens_means_supported: shape gating of the closed-form lens kernels (N <= 224, dk 16 / 32 / 64, L <= 4, L V <= 16, LDS budget)"""
    from mop_amd import _lib
    a = _lib.LensMeansArgs()
    a.B, a.H, a.N, a.dk, a.V, a.L = 2, 6, 197, 64, 5, 2
    a.dil[0], a.dil[1] = 1, 2
    assert lib.mopk_lens_means_supported(C.byref(a), 0) == 1 and lib.mopk_lens_means_supported(C.byref(a), 1) == 1
    a.N = 225
    assert lib.mopk_lens_means_supported(C.byref(a), 0) == 0
    a.N, a.dk = 197, 48
    assert lib.mopk_lens_means_supported(C.byref(a), 0) == 0
    a.dk, a.V, a.L = 64, 5, 4                      # L V = 20 channels
    for i in range(4):
        a.dil[i] = 1
    assert lib.mopk_lens_means_supported(C.byref(a), 0) == 0
    a.V, a.L, a.N = 4, 4, 224                      # 16 channels: the backward's working set grows with the largest dilation
    assert lib.mopk_lens_means_supported(C.byref(a), 1) == 1
    a.dil[3] = 200
    assert lib.mopk_lens_means_supported(C.byref(a), 0) == 1 and lib.mopk_lens_means_supported(C.byref(a), 1) == 0
    a.dil[3] = 0
    assert lib.mopk_lens_means_supported(C.byref(a), 0) == 0
    assert lib.mopk_lens_means_fwd(None, None) < 0 and lib.mopk_lens_means_bwd(None, None) < 0


def test_bad_args_are_rejected_before_any_launch(lib):
    from mop_amd import _lib
    a = _lib.EdgewiseArgs()
    assert lib.mopk_edgewise_lowrank_fwd(C.byref(a), None) == -1  # bad shape
    a.B, a.H, a.N, a.dk, a.V, a.r = 1, 1, 8, 16, 2, 2
    assert lib.mopk_edgewise_lowrank_fwd(C.byref(a), None) == -2  # null pointers
