"""No GPU: the case table of tests/test_gpu_prefill_rows.py (tests/prefill_rows_cases.py), its checker and its bars, on the oracle alone.

  * the table holds what it claims: stream lengths, a padding row and an utterance boundary inside a GEMM block, an utterance across every
    pass boundary, every valid row mapped exactly once, the block-GEMM form of every matrix as launch_blk / launch_blk_e / plan_pass
    decide it, and every form under every epilogue it can reach;
  * the checker finds what the last-row instrument misses: four defect models applied inside the oracle (RowsOracle.defect) - the
    checker flags exactly the damaged rows at the first layer that shows them and nothing outside their causal cone afterwards, while
    the relative L2 of every utterance's LAST logits row (what every other parity test reads) stays under the 2e-2 bar;
  * the fp32 bar is not met by luck: the oracle in fp64 against itself in fp32 stays inside it on every case of the two tiny widths."""
import dataclasses

import numpy as np
import pytest
import torch

import prefill_rows_cases as pc

STREAMS = {"e-small": 272, "e-sbs-512": 1808, "e-sbs-512-full": 2048, "e-sbs-512-edge": 1792, "e-sbs-2048": 400, "e-big-1024": 1024,
           "e-big-1040": 1040, "e-big-1552": 1552, "e-big-2048": 2048, "e-pass-tiny128-fp32": 2304, "e-pass-giga-bf16": 1552,
           "p-tts": 224, "p-tts-bf16-attn64": 256, "p-multi-tiny128": 1808, "p-multi-giga": 1904, "e-sbs-1280": 656, "e-big-1792": 1296}


def _stream_of(name):
    return STREAMS[max((k for k in STREAMS if name.startswith(k)), key=len)]


def test_the_table_holds_what_it_claims():
    seen = set()
    for c in pc.CASES:
        lay = pc.layout(c.name)
        a, _ = pc.model(c.preset)
        assert a.num_decoder_layers == 2
        if c.family != "edit":
            assert c.stream == lay.R == _stream_of(c.name), (c.name, c.stream)
        assert c.stream <= pc.MAX_ROWS or len(c.pass_rows) > 1
        assert c.B <= c.seqs and max(c.rows) + 8 <= c.max_positions
        # every valid row exactly once, padding rows nowhere
        pairs = {(int(u), int(p)) for u, p in zip(lay.utt[lay.valid], lay.pos[lay.valid])}
        assert len(pairs) == int(lay.valid.sum()) == sum(c.rows) and pairs == {(u, p) for u, n in enumerate(c.rows) for p in range(n)}, c.name
        assert (lay.utt[~lay.valid] == -1).all() and all(r % c.align == 0 for r in lay.row0)
        # the forms, as the engine's rules give them
        assert pc.derived_forms(c) == c.forms, (c.name, pc.derived_forms(c))
        assert len(c.forms) == len(c.pass_rows)
        big = c.dtype == "bf16" and a.d_model in (1792, 2048)          # (d = 1792: the odd width at which big256 is cheapest, e-big-1792)
        for f, rows in zip(c.forms, c.pass_rows):
            assert (pc.BIG in f) <= (big and rows > 1024), (c.name, f)
            seen |= {(f[1], f[0]), (f[2], "PART"), (f[3], "RELU"), (f[4], "PART")}
        if c.family == "eval" and c.B > 1:
            blk = pc.BIG_M if pc.BIG in c.forms[0] else pc.BLK_M
            mixed = [b for b in range(0, lay.R, blk) if len(set(lay.utt[b: b + blk]) - {-1}) > 1]
            assert mixed, (c.name, "no utterance boundary inside a block")
            assert any((~lay.valid[b: b + blk]).any() and lay.valid[b: b + blk][np.flatnonzero(~lay.valid[b: b + blk])[0]:].any() for b in mixed), \
                (c.name, "no padding row with valid rows behind it inside a block")
        edge = 0
        for rows in c.pass_rows[:-1]:                       # an utterance on both sides of every pass boundary
            edge += rows
            assert lay.utt[edge - 1] == lay.utt[edge] >= 0, (c.name, edge)
        if c.family == "eval":
            assert ((lay.tgt >= 0).any(axis=1) <= (lay.pos >= np.array(lay.Lx + (0,))[lay.utt])).all(), "text rows carry no target"
    for form in ("blk64", pc.SBS, pc.BIG):
        for epi in ("QKV", "QKV16", "PART", "RELU"):
            assert (form, epi) in seen, (form, epi)
    # the odd widths: every preset on blk64, and each further form at the smallest stream that takes it at its width (one tile less: not yet)
    assert {c.preset for c in pc.CASES if c.name.startswith("e-small-w")} == set(pc.ODD_PRESETS)
    for name, form in (("e-sbs-1280-fp32", pc.SBS), ("e-big-1792", pc.BIG)):
        c = pc.BY_NAME[name]
        shorter = dataclasses.replace(c, name="shorter", rows=(c.stream - 16,))
        assert form in c.forms[0] and form not in pc.derived_forms(shorter)[0] and c.preset in pc.ODD_PRESETS, name
    small = pc.layout("e-small-tiny128-fp32")
    assert int(small.valid[256:].sum()) == 3 and small.R - 256 == 16, "the last block: one tile with three valid rows"
    multi = [c for c in pc.CASES if len(c.pass_rows) > 1]
    assert {(c.preset, c.dtype) for c in multi} == {("tiny128", "fp32"), ("giga830M", "bf16")}
    assert any("prefill_rows" not in dict(c.options) for c in multi) and any(dict(c.options).get("prefill_rows") == "1040" for c in multi)


def test_the_rows_keyed_loss_is_the_oracles_loss():
    """The recording oracle's rows are the oracle's own numbers: the per-row terms, summed, are VoiceCraft.forward's loss, and the logits
    columns are the ones its revert reads (`_per_token_logits`)."""
    name = "e-small-tiny128-fp32"
    a, sd = pc.model("tiny128")
    batch, spans = pc.eval_batch(name)
    out = pc.VoiceCraftOracle(a, sd).forward(batch, spans)
    ref, lay = pc.reference(name), pc.layout(name)
    assert abs(float(ref["nll"].astype(np.float64).sum()) - float(out["loss"])) <= 1e-5 * float(out["loss"])
    assert int((lay.tgt >= 0).sum()) == int(out["effective_ntoken"])
    assert out["_logits_cols"].shape[:2] == (3, a.n_codebooks)
    assert np.array_equal(np.sort(pc.own_nll(ref["logits"], lay.tgt)[lay.tgt >= 0]),
                          np.sort(torch.nn.functional.cross_entropy(out["_per_token_logits"].double().reshape(-1, out["_per_token_logits"].shape[-1]),
                                                                    out["_targets"].reshape(-1), reduction="none").numpy()))


# engine coordinates: (kind, layer, utterance, position, ...); rows of e-small: utterance 0 at 0, 1 at 112, 2 at 192
DEFECTS = {
    "a: two rows swapped inside one tile (FFN-down, layer 0)": (("swap", 0, 1, 18, 21), [(1, 18), (1, 21)]),
    "a': the same behind the last layer": (("swap", 1, 1, 18, 21), [(1, 18), (1, 21)]),
    "b: a row replaced by the row 128 before it (FFN-down, layer 0)": (("copy", 0, 2, 32, 0, 96), [(2, 32)]),
    "c: a 256-wide K chunk dropped from one row (FFN-down, layer 0)": (("chunk", 0, 0, 50, 256), [(0, 50)]),
    "d: a row's K/V written to the neighbouring slot (layer 1)": (("slot", 1, 1, 40, 2), [(1, 40), (2, 40)]),
}


@pytest.mark.parametrize("label", list(DEFECTS))
def test_the_checker_flags_the_damaged_rows_and_the_last_row_instrument_does_not(label):
    name = "e-small-tiny128-fp32"
    defect, hit = DEFECTS[label]
    lay, clean = pc.layout(name), pc.reference(name)
    got = pc.oracle_rows(name, defect=defect)
    row = {(int(u), int(p)): r for r, (u, p) in enumerate(zip(lay.utt, lay.pos)) if p >= 0}
    D = sorted(row[h] for h in hit)
    if defect[0] == "copy":
        assert D[0] - row[(defect[4], defect[5])] == 128
    if defect[0] == "swap":
        assert D[0] // 16 == D[1] // 16
    cone = {r for r in range(lay.R) if any(lay.utt[r] == u and lay.pos[r] >= p for u, p in hit)}
    l0 = defect[1]
    first_kv = l0 if defect[0] == "slot" else l0 + 1          # a damaged hidden row shows in the NEXT layer's K/V; a scatter in its own
    for dtype in ("fp32", "bf16"):
        kv_n, kv_fig = 0, 0.0
        for l in range(2):
            for which in ("k", "v"):
                bad, _, f = pc.check_rows(got[which][l], clean[which][l], dtype, lay.valid)
                bad, kv_n, kv_fig = list(bad), kv_n + len(bad), max(kv_fig, f)
                if l < first_kv:
                    assert bad == [], (label, dtype, which, l, bad)
                elif l == first_kv:
                    assert bad == D, (label, dtype, which, l, bad, D)          # exactly the damaged rows
                else:
                    assert set(bad) <= cone, (label, dtype, which, l, bad)
        bad, worst, fig = pc.check_rows(got["logits"], clean["logits"], dtype, clean["has_logits"], logits=True)
        assert set(bad) <= cone, (label, dtype, bad)
        if defect[0] != "slot":
            assert clean["has_logits"][D].all() and set(D) <= set(bad), (label, dtype, bad, D)      # the damaged hidden rows reach their own logits rows
        # today's instrument: the head logits of each utterance's last row
        last = [lay.row0[u] + n - 1 for u, n in enumerate(pc.BY_NAME[name].rows)]
        inst = pc.row_error(got["logits"][last], clean["logits"][last], "bf16")
        if dtype == "bf16":
            print(f"{label}: flagged K/V rows {kv_n}, worst {kv_fig:.3g}; flagged logits rows {len(bad)}, worst {fig:.3g}; last-row logits rel L2 {inst.max():.2e} against the bar {pc.BAR_BF16:.0e}")
            assert inst.max() < pc.BAR_BF16, (label, inst)


FP64 = [c.name for c in pc.CASES if c.dtype == "fp32" and c.preset != "giga830M" and c.name != "e-pass-tiny128-fp32-1040"]


@pytest.mark.parametrize("name", FP64)
def test_the_fp32_oracle_meets_the_fp32_bar_against_fp64(name):
    """(giga width is left out for its CPU time; e-pass at 1 040 rows per pass has the oracle run of the default pass size.)"""
    lay, r32 = pc.layout(name), pc.reference(name)
    r64 = pc.oracle_rows(name, dtype=torch.float64)
    worst = {}
    for l in range(2):
        for which in ("k", "v"):
            bad, _, worst[f"{which}{l}"] = pc.check_rows(r32[which][l], r64[which][l], "fp32", lay.valid)
            assert len(bad) == 0, (name, which, l, bad[:8])
    assert np.abs(r32["emb"] - r64["emb"]).max() <= 1e-5
    if "logits" in r32:
        bad, _, worst["logits"] = pc.check_rows(r32["logits"], r64["logits"], "fp32", r32["has_logits"], logits=True)
        assert len(bad) == 0, (name, "logits", bad[:8])
        worst["nll"] = float((pc.nll_error(r32["nll"], r64["nll"]) * (lay.tgt >= 0)).max())
        assert worst["nll"] <= pc.BAR_NLL, (name, worst)
    print(f"{name}: fp32 oracle against fp64, worst per quantity {({k: float(f'{v:.3g}') for k, v in worst.items()})}")
    assert max(v for k, v in worst.items() if k != "nll") <= 0.01 * pc.BAR_F32, (name, worst)      # the oracle's own rounding: 100 x inside the bar
