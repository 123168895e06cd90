"""Decode rows through the whole step: the cases of tests/test_gpu_decode_rows.py, their inputs, the references and the
defect model.  No GPU in this module; tests/test_decode_rows_cpu.py checks the plan table, the geometry and the bar.

tests/test_gpu_decode_attn.py holds rows_attn_k itself to float64.  What it cannot see is what happens to the kernel's partials in a
decode step: the merging prologues of the out-projection (PRO_ATT of rows_gemm_k on slabs; rows_gemm_fr_k at 2 / 4 / 8 splits with
fp32 or bf16 partials), the hand-over of the normalised rows from unsplit launches, and the QKV epilogue's cache write at decode
positions.  Here a call is teacher-forced from its prompt until its cache is full, and K and V of layers 1 and 2 (tiny128 at THREE
decoder layers) are read back from the cache at EVERY decode position: layer l + 1's K/V row at a position is a linear image of what
layer l's attention, out-projection and FFN made of that row.

A case is (dtype, rows per step).  The rows per step pick the form (vc_debug_plan): 1 row 8 splits on slabs; 2 rows 8 splits, 4 rows 4
splits, 8 rows 2 splits, 12 rows unsplit, all on finished rows; 20 rows the wide form.  max_positions = (nsplit + 2) * 4 * 8 * PPW
(head_dim 128: PPW = 2 in fp32, 4 in bf16), i.e. 640 / 1280 for the one- and two-row steps, so that the longest context, max_positions
- 2, lies a whole batch and more past the first refill of every split.  (A call keeps one position spare and feeds its last token to
nobody: the last step WRITES position max_positions - 3 at most, vc_engine.hip `room`.)  The step budget of a call is ten frames per
phoneme, so a call that fills 1280 positions needs a text of ~120 phonemes: the prompts are a long text and eight frames.

Reference: RowsOracle in float64 through tts_logits_for_trajectory - one causal pass over [text ; prompt columns ; forced tokens],
which records K/V of every row.  Bars:
  fp32   per row max|d| <= 16 x the worst per-row distance of the FP32 oracle from the float64 oracle over the same rows (both runs are
         part of the case's reference): the engine sums in another order than ATen, nothing else.
  bf16   relative L2 per row <= 2e-2, the project's bf16 bar.  That sees a wrong slot, a missing partial or a stale row - not one
         position; the position-level evidence for bf16 is tests/test_gpu_decode_attn.py.
Defect model (DropOracle): layer l's attention at ONE row ignores ONE position (one -inf in the one-pass mask); the CPU test shows that
at the longest fp32 context it moves layer l + 1's K/V row by more than 4 bars wherever the position lies."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch

import decode_attn_cases as dc
import prefill_rows_cases as pc

PRESET, LAYERS, SEED, T_PROMPT = "tiny128", 3, 11, 8
FORM_SLAB, FORM_FR, FORM_WIDE = 0, 1, 2
PLAN = {1: (FORM_SLAB, 8), 2: (FORM_FR, 8), 4: (FORM_FR, 4), 8: (FORM_FR, 2), 12: (FORM_FR, 1), 20: (FORM_WIDE, 1)}      # rows: (form, splits)
CASES = [(dtype, rows) for dtype in dc.DTYPES for rows in PLAN]
BAR_BF16 = 2e-2
ORACLE_X = 16.0           # fp32 bar = ORACLE_X x the fp32 oracle's own error
DEFECT_X = 4.0


@functools.lru_cache(maxsize=None)
def model():
    from voicecraft_amd import synth
    a = synth.make_args(PRESET, num_decoder_layers=LAYERS)
    return a, synth.make_state_dict(a, seed=SEED)


def plan(dtype, rows):
    """(form, attention splits) of a decode step of `rows` rows, from vc_debug_plan."""
    from voicecraft_amd import _lib
    out = (C.c_int32 * 16)()
    cfg = pc.model_cfg(model()[0], max_seqs=32, max_positions=1280)
    assert _lib.load().vc_debug_plan(C.byref(cfg), _lib.VC_DTYPE_BF16 if dtype == "bf16" else _lib.VC_DTYPE_F32, rows, out) == 0
    return out[1], out[2]


def max_positions(dtype, rows):
    return (PLAN[rows][1] + 2) * dc.batch(dtype, 128)


@functools.lru_cache(maxsize=None)
def inputs(dtype, rows):
    """(xs, ys, forced [n][rows][K], P): texts of different lengths (so the rows of a step sit at different positions), T_PROMPT frames
    each, and per sequence a random trajectory whose last K steps are the staggered terminator; n fills the cache of the sequence with
    the longest prompt.  P[u] = prompt positions of sequence u = its first decode position."""
    from voicecraft_amd import synth
    a, _ = model()
    S_max = max_positions(dtype, rows)
    lx0 = S_max // 11 + 2
    lens = [lx0 + (3 * u) % 7 for u in range(rows)]
    prompts = [synth.random_prompt(a, lx, T_PROMPT, seed=300 + u) for u, lx in enumerate(lens)]
    P = [lx + T_PROMPT + 1 for lx in lens]
    n = S_max - max(P) - 1
    assert all(lx * 10 - (T_PROMPT + 1) + 1 + a.n_codebooks >= n for lx in lens)          # the call's own step budget
    forced = np.stack([forced_trajectory(a, n, seed=700 + u, term=a.eos) for u in range(rows)], axis=1)
    return [p[0][0] for p in prompts], [p[2][0] for p in prompts], forced, tuple(P)


def forced_trajectory(a, n, seed, term):
    """n steps of random plain codes whose last K steps are the staggered end of a span (tests/test_gpu_scale.py)."""
    K = a.n_codebooks
    toks = np.random.RandomState(seed).randint(0, a.audio_vocab_size, size=(n, K)).astype(np.int64)
    for j in range(K):
        toks[n - K + j, :j] = a.empty_token
        toks[n - K + j, j] = term
    return toks


class DropOracle(pc.RowsOracle):
    """RowsOracle whose layer `drop[0]` attention ignores position drop[2] at row drop[1] (positions of the one causal pass)."""

    def __init__(self, args, state_dict, dtype=torch.float32, drop=None):
        super().__init__(args, state_dict, dtype)
        self.drop = drop

    def _attn(self, l, x, mask, past_l):
        if self.drop is not None and self.drop[0] == l and past_l is None:
            mask = mask.clone()
            mask[:, :, self.drop[1], self.drop[2]] = float("-inf")
        return super()._attn(l, x, mask, past_l)


def oracle_kv(dtype, rows, u, torch_dtype=torch.float64, drop=None):
    """K/V rows of sequence u, every position the call writes: {"k" / "v": [LAYERS][positions, d]} in float64 numpy."""
    a, sd = model()
    xs, ys, forced, P = inputs(dtype, rows)
    orc = DropOracle(a, sd, torch_dtype, drop)
    n = forced.shape[0]
    orc.tts_logits_for_trajectory(xs[u].unsqueeze(0), ys[u].unsqueeze(0), forced[:, u], steps=[n - 1])
    out = {"k": [], "v": []}
    for l in range(LAYERS):
        for key, t in zip(("k", "v"), orc.rec[l]):
            S = t.shape[2]
            out[key].append(t[0].permute(1, 0, 2).reshape(S, a.d_model).double().numpy())          # [H, S, hd] -> head-major rows
    assert S == P[u] + n - 1
    return out


def row_abs(got, want):
    """Per row: the largest |d| (anything that is not a number counts as infinitely far)."""
    d = np.abs(np.asarray(got, np.float64) - want)
    return np.where(np.isfinite(d), d, np.inf).max(axis=1)


def row_rel(got, want):
    """Per row: the relative L2 distance."""
    d = np.asarray(got, np.float64) - want
    d = np.where(np.isfinite(d), d, np.inf)
    return np.sqrt((d ** 2).sum(axis=1)) / np.sqrt((want ** 2).sum(axis=1))


@functools.lru_cache(maxsize=2)
def reference(dtype, rows):
    """Per sequence the float64 K/V rows, and for fp32 cases the fp32 oracle's worst per-row distance from them over the decode rows of
    layers 1 .. LAYERS - 1 (`oracle_err`) and the bar ORACLE_X times that."""
    xs, ys, forced, P = inputs(dtype, rows)
    ref = [oracle_kv(dtype, rows, u) for u in range(rows)]
    err = 0.0
    if dtype == "fp32":
        for u in range(rows):
            o32 = oracle_kv(dtype, rows, u, torch.float32)
            for l in range(1, LAYERS):
                for key in ("k", "v"):
                    err = max(err, float(row_abs(o32[key][l][P[u]:], ref[u][key][l][P[u]:]).max()))
    return dict(kv=ref, oracle_err=err, bar=ORACLE_X * err)
