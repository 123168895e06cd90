"""Decode steps at the model widths that are no power of two: the cases of tests/test_gpu_odd_widths.py, their inputs, the
references, the bars and the defect models.  No GPU in this module; tests/test_odd_widths_cpu.py checks the plan table, the bars and what
the defect models move.

Every other test that runs a model on the GPU has d = 256 / 512 / 1024 / 2048 and 4 or 16 heads.  At d = 768 / 1280 / 1536 / 1792 the
decode kernels take text that no such width reaches: the staging prologues divide where they otherwise shift (x_upr_shift / att_q4_shift
= -1), a wave of the finished-row producers owns 3 / 5 / 7 k-chunks instead of one, the one-row kernel runs its non-EXACT form (clamped
pair addresses, zeroed fragments), the paired forms are off (frp = qp = 0), 17..64-row steps fall back to rows_gemm_mt_k (wd = 0), steps
of fr_max_rows + 1 .. 16 rows run on slabs with 2 .. 7 attention splits, and the head counts 10 .. 56 enter the head / element arithmetic
of the merges, of the QKV epilogue's cache write and of the attention grids.

A case is (preset, dtype, rows per step).  For each (preset, dtype) the row counts are the first of every maximal run of equal
vc_debug_plan vectors over 1 .. 20 rows, and 16 and 20 (`derived_rows`); PLAN states them by hand with the form and the attention splits
of each, and the CPU test holds the two against each other, so that a planner change has to be acknowledged here.

Inputs: per preset N_SEQ sequences, sequence u with a text of 12 + (3 u) % 7 phonemes, T_PROMPT prompt frames and a forced trajectory of
N_STEPS steps whose last K are the staggered terminator, so every sequence of a call ends at the same step and a call of `rows` rows
(sequences 0 .. rows - 1) has `rows` rows in every decode step.  Prompts are 21 .. 27 positions, contexts of decode rows 22 .. 38.

Reference: RowsOracle in float64 through tts_logits_for_trajectory, one causal pass per sequence, computed once per preset and shared by
its cases: K and V of layer 1 at every position (prompt and decode) and the head logits [K, V] of every step.  Bars:
  fp32   per row max|d| over the live entries (|want| < 1e3) <= ORACLE_X = 16 x the worst per-row distance of the FP32 oracle from the
         float64 one over the same rows (the case's sequences), separately for K/V rows and logits rows; and the arg-max of every
         (step, codebook) equals the float64 one except where the float64 top-two margin is below the logits bar.  Such exceptions are
         capped at 1 % of the preset's (sequence, step, codebook) triples; the CPU test holds the fp32 oracle alone to the same rule.
  bf16   relative L2 per row <= 2e-2 over the live entries, the project's bf16 bar, for K/V rows and logits rows.

Defect models (OddOracle, layer 0, one decode row of the one causal pass):
  ("ffn", r, k0, k1) / ("out", r, k0, k1)   the FFN down-projection / the out-projection loses the k-chunk [k0, k1) of its reduction -
                                            a share K / nchunk as vc_launch_gemm_fr cuts it (`fr_nchunk`), the first and the last
  ("head", r)                               the attention output of head H - 1 is replaced by head 0's (a wrong h_ in a merge)
  ("split", r, p0, p1)                      the attention ignores the positions of one split's chunk (decode_attn_cases.splits)
What the bars see (tests/test_odd_widths_cpu.py prints the figures, profiles/odd_widths_pytest_cpu.log): every model moves layer 1's
K/V row or a logits row by 1 900 .. 12 000 fp32 bars at every preset (DEFECT_X = 4 is asked).  The bf16 bar of 2e-2 SEES a dropped
k-chunk, with little room (one of 3 chunks 2.4 .. 3.5 bars, one of 5 1.8 .. 2.7, one of 7 1.4 .. 2.3), and a wrong head at 10 .. 24 heads
(1.2 .. 1.8 bars); it does NOT see a wrong head among 56 (0.73 bars) and does not reliably see a dropped split of eight (0.74 .. 1.15
bars), let alone anything finer.  The bf16 arm therefore holds whole-chunk and whole-row damage (a wrong slot, a stale or missing row,
a missing residual); the head- and split-level evidence at these widths is the fp32 arm, which runs the same kernel text with the other
element size, and for the attention kernel itself tests/test_gpu_decode_attn.py.  The contexts are 22 .. 38 positions under the
kernel's chunk rule ceil(S / n): at some of them the last one or two of 6 / 7 / 8 splits hold no position (S = 25 with n = 8: seven
chunks of 4), so the merges' arm for a partial without positions runs here too; the CPU test lists where."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch
import torch.nn.functional as F

import decode_attn_cases as dc
import decode_rows_cases as dr
import prefill_rows_cases as pc

PRESETS = ("w768_h12", "w768_h24", "w1280_h10", "w1536_h24", "w1792_h14", "w1792_h56")
DTYPES = ("fp32", "bf16")
N_SEQ, T_PROMPT, N_STEPS, MAX_POSITIONS = 20, 8, 12, 128
MAX_SEQS = N_SEQ              # of the test engine, and of the plan that is asked for
FORM_SLAB, FORM_FR, FORM_WIDE = dr.FORM_SLAB, dr.FORM_FR, dr.FORM_WIDE
BAR_BF16 = 2e-2
ORACLE_X = 16.0               # fp32 bar = ORACLE_X x the fp32 oracle's own distance from the float64 oracle
DEFECT_X = 4.0
ARGMAX_CAP = 0.01             # of the preset's (sequence, step, codebook) triples

S, R, W = FORM_SLAB, FORM_FR, FORM_WIDE
# (preset, dtype): {rows: (form, attention splits)} - vc_debug_plan out[1], out[2] at max_seqs = 20
PLAN = {
    ("w768_h12", "fp32"): {1: (S, 8), 2: (R, 8), 3: (R, 4), 5: (R, 2), 9: (R, 1), 11: (S, 3), 15: (S, 2), 16: (S, 2), 17: (W, 1), 20: (W, 1)},
    ("w768_h12", "bf16"): {1: (S, 8), 2: (R, 8), 3: (R, 4), 5: (R, 2), 9: (R, 1), 16: (R, 1), 17: (W, 1), 20: (W, 1)},
    ("w768_h24", "fp32"): {1: (S, 8), 2: (R, 8), 3: (R, 4), 5: (R, 2), 9: (R, 1), 11: (S, 1), 16: (S, 1), 17: (W, 1), 20: (W, 1)},
    ("w768_h24", "bf16"): {1: (S, 8), 2: (R, 8), 3: (R, 4), 5: (R, 2), 9: (R, 1), 16: (R, 1), 17: (W, 1), 20: (W, 1)},
    ("w1280_h10", "fp32"): {1: (S, 8), 2: (R, 8), 3: (R, 4), 5: (R, 2), 7: (S, 7), 8: (S, 6), 9: (S, 5), 11: (S, 4), 13: (S, 3), 16: (S, 3),
                            17: (W, 1), 20: (W, 1)},
    ("w1280_h10", "bf16"): {1: (S, 8), 2: (R, 8), 3: (R, 4), 5: (R, 2), 9: (R, 1), 13: (S, 3), 16: (S, 3), 17: (W, 1), 20: (W, 1)},
    ("w1536_h24", "fp32"): {1: (S, 8), 2: (R, 8), 3: (R, 4), 5: (R, 2), 6: (S, 3), 8: (S, 2), 11: (S, 1), 16: (S, 1), 17: (W, 1), 20: (W, 1)},
    ("w1536_h24", "bf16"): {1: (S, 8), 2: (R, 8), 3: (R, 4), 5: (R, 2), 9: (R, 1), 11: (S, 1), 16: (S, 1), 17: (W, 1), 20: (W, 1)},
    ("w1792_h14", "fp32"): {1: (S, 8), 2: (R, 8), 3: (R, 4), 5: (S, 7), 6: (S, 6), 7: (S, 5), 8: (S, 4), 10: (S, 3), 13: (S, 2), 16: (S, 2),
                            17: (W, 1), 20: (W, 1)},
    ("w1792_h14", "bf16"): {1: (S, 8), 2: (R, 8), 3: (R, 4), 5: (R, 2), 9: (R, 1), 10: (S, 3), 13: (S, 2), 16: (S, 2), 17: (W, 1), 20: (W, 1)},
    ("w1792_h56", "fp32"): {1: (S, 4), 2: (R, 4), 3: (R, 2), 5: (S, 1), 16: (S, 1), 17: (W, 1), 20: (W, 1)},
    ("w1792_h56", "bf16"): {1: (S, 4), 2: (R, 4), 3: (R, 2), 5: (R, 2), 9: (R, 1), 10: (S, 1), 16: (S, 1), 17: (W, 1), 20: (W, 1)},
}
del S, R, W
CASES = [(preset, dtype, rows) for preset in PRESETS for dtype in DTYPES for rows in PLAN[(preset, dtype)]]


def model(preset):
    """(args, state dict) of a preset at two layers: the models of tests/prefill_rows_cases.py (drawn with fast=True above d = 512)."""
    return pc.model(preset)


def plan_vector(preset, dtype, rows):
    """vc_debug_plan's 16 numbers for a decode step of `rows` rows at the test engine's max_seqs."""
    from voicecraft_amd import _lib
    out = (C.c_int32 * 16)()
    cfg = pc.model_cfg(model(preset)[0], max_seqs=MAX_SEQS, max_positions=MAX_POSITIONS)
    assert _lib.load().vc_debug_plan(C.byref(cfg), _lib.VC_DTYPE_BF16 if dtype == "bf16" else _lib.VC_DTYPE_F32, rows, out) == 0
    return tuple(out)


def derived_rows(preset, dtype):
    """{rows: (form, splits)}: the first row count of every maximal run of equal plan vectors over 1 .. 20 rows, and 16 and 20."""
    vec = {rows: plan_vector(preset, dtype, rows) for rows in range(1, N_SEQ + 1)}
    take = {rows for rows in vec if rows == 1 or vec[rows] != vec[rows - 1]} | {16, 20}
    return {rows: (vec[rows][1], vec[rows][2]) for rows in sorted(take)}


def fr_nchunk(K, dtype):
    """vc_launch_gemm_fr: k-chunks per wave of a finished-row producer over a reduction of K (8 waves, k-tiles of 32 bf16 / 16 fp32
    elements, the largest power of two of k-tiles per wave and chunk up to 32)."""
    KT, ktw = K // (32 if dtype == "bf16" else 16), 32
    while ktw > 1 and KT % (8 * ktw):
        ktw //= 2
    assert KT % (8 * ktw) == 0, (K, dtype)
    return KT // (8 * ktw)


@functools.lru_cache(maxsize=None)
def inputs(preset):
    """(xs, ys, forced [N_STEPS][N_SEQ][K], P): P[u] = prompt positions of sequence u = its first decode position."""
    from voicecraft_amd import synth
    a, _ = model(preset)
    lens = [12 + (3 * u) % 7 for u in range(N_SEQ)]
    prompts = [synth.random_prompt(a, lx, T_PROMPT, seed=300 + u) for u, lx in enumerate(lens)]
    P = tuple(lx + T_PROMPT + 1 for lx in lens)
    assert all(lx * 10 - (T_PROMPT + 1) + 1 + a.n_codebooks >= N_STEPS for lx in lens)              # the call's own step budget
    assert max(P) + N_STEPS - 1 + 3 <= MAX_POSITIONS
    forced = np.stack([dr.forced_trajectory(a, N_STEPS, seed=700 + u, term=a.eos) for u in range(N_SEQ)], axis=1)
    forced.setflags(write=False)
    return [p[0][0] for p in prompts], [p[2][0] for p in prompts], forced, P


def positions(preset, u):
    """Positions a call writes for sequence u: the prompt and the tokens of steps 0 .. N_STEPS - 2."""
    return inputs(preset)[3][u] + N_STEPS - 1


class OddOracle(pc.RowsOracle):
    """RowsOracle with the defect models of the module docstring in `self.odd` (layer 0, row r of the one causal pass, batch index 0)."""

    def __init__(self, args, state_dict, dtype=torch.float32):
        super().__init__(args, state_dict, dtype)
        self.odd = None

    def set_defect(self, odd):
        self.odd = odd
        self.defect = ("chunk", 0, 0, odd[1], odd[2], odd[3] - odd[2]) if odd and odd[0] == "ffn" else None

    def _attn(self, l, x, mask, past_l):
        odd = self.odd if l == 0 and past_l is None else None
        if odd and odd[0] == "split":
            mask = mask.clone()
            mask[:, :, odd[1], odd[2]: odd[3]] = float("-inf")
        if not odd or odd[0] not in ("head", "out"):
            return super()._attn(l, x, mask, past_l)
        # RowsOracle._attn without a cache, with a hand between the attention and its out-projection
        p = f"decoder.layers.{l}.self_attn."
        B, n, d = x.shape
        H, hd = self.H, self.hd
        proj = F.linear(x.transpose(1, 0), self.sd[p + "in_proj_weight"], self.sd[p + "in_proj_bias"])
        proj = proj.unflatten(-1, (3, d)).unsqueeze(0).transpose(0, -2).squeeze(-2).contiguous()
        q, k, v = (t.view(n, B * H, hd).transpose(0, 1).view(B, H, n, hd) for t in (proj[0], proj[1], proj[2]))
        self.rec[l] = (k.clone(), v.clone())
        o = F.scaled_dot_product_attention(q, k, v, mask, 0.0, is_causal=False)
        r = odd[1]
        if odd[0] == "head":
            o = o.clone()
            o[0, H - 1, r] = o[0, 0, r]
        o = o.permute(2, 0, 1, 3).contiguous().view(B * n, d)
        W = self.sd[p + "out_proj.weight"]
        out = F.linear(o, W, self.sd[p + "out_proj.bias"])
        if odd[0] == "out":
            assert B == 1
            out[r] = out[r] - W[:, odd[2]: odd[3]] @ o[r, odd[2]: odd[3]]
        return out.view(n, B, d).transpose(1, 0), torch.stack([k, v], dim=0)


def oracle_seq(orc, preset, u):
    """One causal pass of sequence u: (k [S, d], v [S, d] of layer 1, logits [N_STEPS, K, V]) in float64 numpy, S = positions(preset, u)."""
    a, _ = model(preset)
    xs, ys, forced, P = inputs(preset)
    orc.rec = {}
    lg = orc.tts_logits_for_trajectory(xs[u].unsqueeze(0), ys[u].unsqueeze(0), forced[:, u].copy(), steps=range(N_STEPS))
    k, v = (t[0].permute(1, 0, 2).reshape(t.shape[2], a.d_model).double().numpy() for t in orc.rec[1])          # [H, S, hd] -> head-major rows
    assert k.shape[0] == positions(preset, u) and lg.shape[:2] == (N_STEPS, a.n_codebooks)
    return k, v, lg.double().numpy()


def make_oracle(preset, torch_dtype):
    return OddOracle(*model(preset), torch_dtype)


@functools.lru_cache(maxsize=2)
def reference(preset):
    """Per sequence the float64 rows (`k`, `v`: [S, d]; `lg`: [N_STEPS, K, V]), the fp32 oracle's rows (`k32`, `v32`, `lg32`), its worst
    per-row distance from the float64 rows (`err_kv[u]`, `err_lg[u]`), the float64 arg-max [N_STEPS, K] and top-two margin."""
    o64, o32 = make_oracle(preset, torch.float64), make_oracle(preset, torch.float32)
    ref = dict(k=[], v=[], lg=[], k32=[], v32=[], lg32=[], err_kv=[], err_lg=[], top=[], margin=[])
    for u in range(N_SEQ):
        k, v, lg = oracle_seq(o64, preset, u)
        k32, v32, lg32 = oracle_seq(o32, preset, u)
        for key, t in zip(("k", "v", "lg", "k32", "v32", "lg32"), (k, v, lg, k32, v32, lg32)):
            t.setflags(write=False)
            ref[key].append(t)
        ref["err_kv"].append(float(max(pc.row_error(k32, k, "fp32").max(), pc.row_error(v32, v, "fp32").max())))
        ref["err_lg"].append(float(pc.row_error(lg32, lg, "fp32").max()))
        two = np.sort(lg, axis=-1)[..., -2:]
        ref["top"].append(lg.argmax(axis=-1))
        ref["margin"].append(two[..., 1] - two[..., 0])
    return ref


def bars(preset, dtype, rows):
    """(K/V bar, logits bar) of a case of sequences 0 .. rows - 1."""
    if dtype == "bf16":
        return BAR_BF16, BAR_BF16
    ref = reference(preset)
    return ORACLE_X * max(ref["err_kv"][:rows]), ORACLE_X * max(ref["err_lg"][:rows])


def argmax_exceptions(preset, bar_lg, rows=N_SEQ):
    """bool [rows][N_STEPS, K]: the float64 top-two margin is below the logits bar."""
    return [m < bar_lg for m in reference(preset)["margin"][:rows]]


def check_case(preset, dtype, rows, got_k, got_v, got_lg):
    """got_k / got_v: per sequence [S_u, d] of layer 1; got_lg: per sequence [N_STEPS, K, V].  EVERY row of every sequence is compared.
    Returns (failures, report): failures a list of strings (empty = the case holds), report the worst figures and where they lie."""
    ref = reference(preset)
    bar_kv, bar_lg = bars(preset, dtype, rows)
    worst = {"k": (0.0, -1, -1), "v": (0.0, -1, -1), "logits": (0.0, -1, -1)}          # (figure, sequence, position / step)
    fails, n_exc, n_miss = [], 0, 0
    for u in range(rows):
        for key, got, want, bar in (("k", got_k[u], ref["k"][u], bar_kv), ("v", got_v[u], ref["v"][u], bar_kv), ("logits", got_lg[u], ref["lg"][u], bar_lg)):
            assert np.shape(got) == want.shape, (key, u, np.shape(got), want.shape)
            err = pc.row_error(got, want, dtype)
            i = int(err.argmax())
            if err[i] > worst[key][0]:
                worst[key] = (float(err[i]), u, i)
            bad = np.flatnonzero(~(err <= bar))
            if len(bad):
                fails.append(f"{key} of sequence {u}: {len(bad)} rows over the bar {bar:.3g}, first {int(bad[0])} at {err[bad[0]]:.3g}")
        if dtype == "fp32":
            exc = ref["margin"][u] < bar_lg
            miss = np.asarray(got_lg[u]).argmax(axis=-1) != ref["top"][u]
            n_exc, n_miss = n_exc + int(exc.sum()), n_miss + int(miss.sum())
            if (miss & ~exc).any():
                s, k = np.argwhere(miss & ~exc)[0]
                fails.append(f"arg-max of sequence {u}, step {s}, codebook {k}: margin {ref['margin'][u][s, k]:.3g} against the bar {bar_lg:.3g}")
    report = dict(worst=worst, bar_kv=bar_kv, bar_lg=bar_lg, argmax_exceptions=n_exc, argmax_misses=n_miss)
    if dtype == "fp32":
        report.update(oracle_kv=max(ref["err_kv"][:rows]), oracle_lg=max(ref["err_lg"][:rows]))
    return fails, report


def defects(preset, dtype="fp32", u=0, step=6):
    """{label: OddOracle defect} at the row that decode step `step` of sequence u computes (its context: the positions up to it)."""
    a, _ = model(preset)
    d, r = a.d_model, inputs(preset)[3][u] + step - 1
    out = {}
    for name, K in (("ffn", 4 * d), ("out", d)):
        n = fr_nchunk(K, dtype)
        out[f"{name}: first of {n} k-chunks"] = (name, r, 0, K // n)
        out[f"{name}: last of {n} k-chunks"] = (name, r, K - K // n, K)
    out[f"head {a.nhead - 1} reads head 0"] = ("head", r)
    live = [(i, c) for i, c in enumerate(dc.splits(r + 1, 8)) if c[0] < c[1]]
    for i, c in (live[0], live[-1]):
        out[f"split {i} of 8 ignored (positions {c[0]}..{c[1] - 1} of {r + 1})"] = ("split", r) + c
    return out
