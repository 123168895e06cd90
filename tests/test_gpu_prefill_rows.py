"""-m gpu: EVERY row of a prefill pass against the oracle (tests/prefill_rows_cases.py).

Evaluation calls (`forward(_per_row=True)`): K and V of both layers from the cache, the head logits of every audio row, every per-row loss
term keyed by row, the target table and the `emb` arena.  Inference calls (`inference_tts`, `inference_tts_multi`, `inference`): K and V
of both layers at every prompt position after the shortest forced trajectory the call accepts (re-packing moves states and input rows,
never cache rows - vc_tokens.hip repack_k - and `shrink` is off anyway), and the `emb` arena.  Every test asserts the launch census of
its prefill: the block-GEMM form of each of the four matrices, the attention kernel, the LayerNorm launches.  Each case prints its worst
row per quantity and its census."""
import ctypes as C

import numpy as np
import pytest
import torch

import prefill_rows_cases as pc

pytestmark = pytest.mark.gpu

CENSUS = ("blk64", "blk128_sbs", "big256", "tile_attn", "tile_attn64", "ln_rows")


def _engine(c):
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sd = pc.model(c.preset)
    eng = VoiceCraftEngine(a, sd, device="cuda:0", dtype=c.dtype, max_seqs=c.seqs, max_positions=c.max_positions, use_graph=False)
    for k, v in c.options:
        eng.set_option(k, v)
    return eng, a


def _decode_form(a, dtype, rows):
    """vc_debug_plan out[1] of a decode step of `rows` rows: 1 = finished rows (no LayerNorm launch), 0 = slabs."""
    from voicecraft_amd import _lib
    out = (C.c_int32 * 16)()
    cfg = pc.model_cfg(a, max_seqs=64, max_positions=1024)
    assert _lib.load().vc_debug_plan(C.byref(cfg), _lib.VC_DTYPE_BF16 if dtype == "bf16" else _lib.VC_DTYPE_F32, rows, out) == 0
    return out[1]


def _cache_rows(eng, c, a, lay, name):
    """A cache of one layer in the engine's row order: [R, d], padding rows zero."""
    H, hd = a.nhead, a.d_model // a.nhead
    t = eng.debug_read(name, (c.seqs, H, c.max_positions, hd), dtype=torch.float32 if c.dtype == "fp32" else torch.bfloat16).float().numpy()
    out = np.zeros((lay.R, a.d_model), np.float32)
    v = lay.valid
    out[v] = t[lay.utt[v], :, lay.pos[v], :].reshape(int(v.sum()), a.d_model)      # [rows, H, hd] -> head-major rows
    return out


def _check_kv_emb(eng, c, a, lay, ref, report):
    for l in range(a.num_decoder_layers):
        for which in ("k", "v"):
            bad, worst, fig = pc.check_rows(_cache_rows(eng, c, a, lay, f"{which}cache{l}"), ref[which][l], c.dtype, lay.valid)
            report.append(f"{which}{l} worst row {worst} (utterance {lay.utt[worst]}, position {lay.pos[worst]}): {fig:.3g}")
            print(f"{c.name}: {report[-1]}")
            assert len(bad) == 0, (c.name, which, l, bad[:16], worst, fig)
    emb = eng.debug_read("emb", (lay.R, a.d_model)).numpy()
    d = np.abs(emb - ref["emb"]).max(axis=1) * lay.valid
    print(f"{c.name}: emb worst row {int(d.argmax())}: {d.max():.3g}")
    assert d.max() == 0.0, (c.name, int(d.argmax()), float(d.max()))      # fp32 in both modes, written by prompt_k in ATen's order: bit for bit
    assert not emb[~lay.valid].any(), "padding rows of the arena are zero"


def _check_census(c, got, extra_ln=(0,)):
    want = pc.expected_census(c)
    got = {k: got[k] for k in CENSUS}
    print(f"{c.name}: census {got}")
    for k in CENSUS[:-1]:
        assert got[k] == want[k], (c.name, k, got, want)
    assert got["ln_rows"] - want["ln_rows"] in extra_ln, (c.name, got, want, extra_ln)


def _delta(eng, c0):
    c1 = eng.launch_counts()
    return {k: c1[k] - c0[k] for k in c1}


@pytest.mark.parametrize("name", [c.name for c in pc.CASES if c.family == "eval"])
def test_every_row_of_an_evaluation_pass(name):
    c, lay, ref = pc.BY_NAME[name], pc.layout(name), pc.reference(name)
    eng, a = _engine(c)
    batch, spans = pc.eval_batch(name)
    c0 = eng.launch_counts()
    out = eng.forward(batch, spans, _per_row=True)
    _check_census(c, _delta(eng, c0))
    report = []
    _check_kv_emb(eng, c, a, lay, ref, report)
    lg = out["_logit_rows"].numpy()
    assert lg.shape == ref["logits"].shape and out["_nll_rows"].shape[0] == lay.R, (lg.shape, out["_nll_rows"].shape, lay.R)
    bad, worst, fig = pc.check_rows(lg, ref["logits"], c.dtype, ref["has_logits"], logits=True)
    print(f"{name}: logits worst row {worst} (utterance {lay.utt[worst]}, position {lay.pos[worst]}): {fig:.3g}")
    assert len(bad) == 0, (name, "logits", bad[:16], worst, fig)
    # the target table, row by row: indices into y -> tokens
    t = out["_tgt_rows"].cpu().numpy().astype(np.int64)
    flat_y = np.concatenate([y.reshape(-1).numpy() for y in pc.inputs(name)[1]])
    tok = np.where(t >= 0, flat_y[np.clip(t, 0, None)], np.where(t <= -2, -(t + 2), -1))
    assert np.array_equal(tok, lay.tgt), name
    # the loss terms, keyed by row: against the cross-entropy of the engine's own logits row, and in fp32 of the oracle's column
    m = lay.tgt >= 0
    nll = out["_nll_rows"].cpu().numpy()
    own = pc.nll_error(nll, pc.own_nll(lg, lay.tgt)) * m
    print(f"{name}: nll against the engine's own logits rows: worst {own.max():.3g} at row {np.unravel_index(own.argmax(), own.shape)}")
    assert own.max() <= pc.BAR_NLL, (name, float(own.max()))
    assert not nll[~m].any(), "rows and codebooks without a target carry no term"
    if c.dtype == "fp32":
        e = pc.nll_error(nll, ref["nll"]) * m
        print(f"{name}: nll against the oracle: worst {e.max():.3g} at row {np.unravel_index(e.argmax(), e.shape)}")
        assert e.max() <= pc.BAR_NLL, (name, float(e.max()))


@pytest.mark.parametrize("name", [c.name for c in pc.CASES if c.family != "eval"])
def test_every_prompt_row_of_an_inference_call(name):
    c, lay, ref = pc.BY_NAME[name], pc.layout(name), pc.reference(name)
    eng, a = _engine(c)
    L, K = a.num_decoder_layers, a.n_codebooks
    inp = pc.inputs(name)
    xs, ys, forced = inp[0], inp[1], inp[-1]
    kn = dict(top_k=1, top_p=1.0, temperature=1.0)
    c0 = eng.launch_counts()
    if c.family == "tts":
        x, y = xs[0].unsqueeze(0), ys[0].unsqueeze(0)
        eng.inference_tts(x.cuda(), torch.tensor([x.shape[1]]).cuda(), y.cuda(), stop_repetition=3, **kn, _forced=forced[:, 0], _seed=1)
        extra = (0,)                                      # one-row steps launch no LayerNorm
    elif c.family == "multi":
        eng.inference_tts_multi(xs, ys, stop_repetition=3, **kn, _forced=forced, _seed=1)
        per = 0 if _decode_form(a, c.dtype, c.B) == 1 else 2 * L + 1      # slab steps of >= 3 rows: two per layer and one before the heads
        extra = tuple(per * n for n in range(len(forced) + 2))
    else:
        x, y = xs[0].unsqueeze(0), ys[0].unsqueeze(0)
        mi = torch.tensor([inp[2][0]], dtype=torch.int64)
        eng.inference(x.cuda(), torch.tensor([x.shape[1]]).cuda(), y.cuda(), mi, stop_repetition=-1, **kn, _forced=forced[:, 0], _seed=1)
        extra = (0,) if _decode_form(a, c.dtype, 3) == 1 else (0, 2 * L)      # the span switch is one 3-row step
    _check_census(c, _delta(eng, c0), extra)
    _check_kv_emb(eng, c, a, lay, ref, [])
