"""tests/decode_rows_cases.py without a GPU: the row counts plan the forms they are listed for, every case's longest context lies past
the first refill of its split, the reference is what the call computes, and the fp32 bar - 16 times the fp32 oracle's own distance from
the float64 oracle - is less than a quarter of what ONE ignored position does to the next layer's K/V row at the longest fp32 context."""
import numpy as np
import pytest
import torch

import decode_attn_cases as dc
import decode_rows_cases as dr


def test_row_counts_plan_their_forms_and_contexts_pass_the_first_refill():
    for dtype, rows in dr.CASES:
        assert dr.plan(dtype, rows) == dr.PLAN[rows], (dtype, rows, dr.plan(dtype, rows))
        xs, ys, forced, P = dr.inputs(dtype, rows)
        S_max, n, (form, nsplit) = dr.max_positions(dtype, rows), forced.shape[0], dr.PLAN[rows]
        B = dc.batch(dtype, 128)
        longest = max(P) + n - 1                       # positions the last step of the longest sequence reads
        assert longest == S_max - 2 and int(dc.chunk_rule(longest, nsplit)) >= B + B // nsplit, (dtype, rows, longest)
        assert len(set(P)) == min(rows, 7) and min(P) + n - 1 > nsplit * B              # every sequence gets past it, at its own positions
        a = dr.model()[0]
        assert forced.shape == (n, rows, a.n_codebooks) and (forced[: n - a.n_codebooks] < a.audio_vocab_size).all()
        assert [int(forced[n - a.n_codebooks + j, 0, j]) for j in range(a.n_codebooks)] == [a.eos] * a.n_codebooks
    assert (dr.max_positions("fp32", 1), dr.max_positions("bf16", 1), dr.max_positions("bf16", 2)) == (640, 1280, 1280)


def test_the_one_pass_reference_equals_the_cached_decode():
    """tts_logits_for_trajectory's one causal pass over [text ; prompt ; forced tokens] holds the rows of the cached, step-by-step decode:
    the prompt's K/V rows and the last step's logits agree (fp32 oracle both ways)."""
    a, sd = dr.model()
    xs, ys, forced, P = dr.inputs("fp32", 20)
    u, steps = 3, 12
    toks = forced[:steps, u].copy()
    toks[steps - a.n_codebooks:] = dr.forced_trajectory(a, steps, 1, a.eos)[steps - a.n_codebooks:]
    orc = dr.DropOracle(a, sd)
    trace = []
    orc.inference_tts(xs[u].unsqueeze(0), torch.tensor([len(xs[u])]), ys[u].unsqueeze(0), top_k=1, forced=toks, trace=trace)
    one = dr.DropOracle(a, sd)
    lg = one.tts_logits_for_trajectory(xs[u].unsqueeze(0), ys[u].unsqueeze(0), toks, steps=[steps - 1])
    live = trace[-1]["logits"][0].abs() < 1e3
    assert ((lg[0] - trace[-1]["logits"][0]).abs() * live).max() <= 1e-3
    want = one.rec
    assert want[0][0].shape[2] == P[u] + steps - 1 and len(trace) == steps
    # the prefill part of the cached run is recorded by RowsOracle itself: the same rows, and the same logits at the last step
    for l in range(dr.LAYERS):
        for i in (0, 1):
            assert np.abs(orc.rec[l][i].numpy() - want[l][i][:, :, : P[u]].numpy()).max() <= 1e-4


def test_one_ignored_position_exceeds_four_bars_at_the_longest_fp32_context():
    dtype, rows, u = "fp32", 1, 0
    ref = dr.reference(dtype, rows)
    xs, ys, forced, P = dr.inputs(dtype, rows)
    n = forced.shape[0]
    row = P[u] + n - 2                                 # the last row the call writes: the longest context, S = row + 1
    S = row + 1
    assert S == dr.max_positions(dtype, rows) - 2
    print(f"fp32 oracle against float64 over the decode rows of layers 1..{dr.LAYERS - 1}: worst row {ref['oracle_err']:.3g}; bar {ref['bar']:.3g}")
    assert 0 < ref["bar"] < 1e-3                       # tighter than the bar the prefill rows are held to
    where = {0, S // 2, row}
    for p0, p1 in dc.splits(S, 8):
        where |= {p0, p1 - 1}
    low = {}
    for l in range(dr.LAYERS - 1):
        for p in sorted(where):
            bad = dr.oracle_kv(dtype, rows, u, torch.float32, drop=(l, row, p))
            moved = min(float(np.abs(bad[key][l + 1][row] - ref["kv"][u][key][l + 1][row]).max()) for key in ("k", "v"))
            if moved < low.get(l, (np.inf, 0))[0]:
                low[l] = (moved, p)
            # rows the defect cannot reach stay where they were (up to the fp32 oracle's own error)
            assert dr.row_abs(bad["k"][l + 1][:row], ref["kv"][u]["k"][l + 1][:row]).max() <= ref["oracle_err"] * 1.0001
    print(f"one ignored position of {S} at layer l moves layer l + 1's K/V row by at least (l: (|d|, position)) {low}")
    assert min(v[0] for v in low.values()) >= dr.DEFECT_X * ref["bar"], (low, ref["bar"])
