"""-m gpu: option `w13` - one-row steps stream the FFN down-projection (bit 1) and the QKV projection (bit 4)
as exact 13-bit planes of the bf16 weights (vc_gemm_w13.hip, vc_w13.h).  The planes hold the same values, the kernels keep the
prologue, epilogue and summation order of their bf16 twins: teacher-forced head logits are BIT-identical to option off, under the
captured graph and eager, at every width at which the kernels take another form - d = 512 (4-fragment FFN-down shares, QKV not
applicable), d = 1024 (QKV's smallest form, 8-fragment FFN-down shares) and d = 2048 (the benchmark's 16 / 8 fragments per wave) -
and the `w13` census slot counts exactly the launches of the applicable bits."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_STEPS = 12
SHAPES = {"tiny128": None, "tiny_h16": None, "giga330M": 2, "giga830M": 1}      # preset -> decoder layers (None: the preset's own)


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


@functools.lru_cache(maxsize=None)
def _model(preset):
    from voicecraft_amd import synth
    kw = {} if SHAPES.get(preset) is None else {"num_decoder_layers": SHAPES[preset]}
    a = synth.make_args(preset, **kw)
    sd = synth.make_state_dict(a, seed=0, fast=True)
    x, xl, y = synth.random_prompt(a, 6, 20, seed=3)
    K = a.n_codebooks
    toks = np.random.RandomState(17).randint(0, a.audio_vocab_size, size=(N_STEPS, K)).astype(np.int64)
    for j in range(K):                      # the staggered end of the span (voicecraft.py:1057-1066): the call ends with its forced steps
        toks[N_STEPS - K + j, :j] = a.empty_token
        toks[N_STEPS - K + j, j] = a.eos
    return a, sd, (x, xl, y), toks


def _logits(eng, prompt, toks):
    x, xl, y = prompt
    _, _, lg = eng.inference_tts(x.cuda(), xl.cuda(), y.cuda(), top_k=1, stop_repetition=3, _forced=toks, _logit_steps=len(toks))
    return lg.cpu().numpy()


def _applicable(d):
    return (1 if d >= 512 else 0) | (4 if d >= 1024 else 0)


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("preset", list(SHAPES))
def test_w13_logits_bit_identical_and_census(preset, use_graph):
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sd, prompt, toks = _model(preset)
    eng = VoiceCraftEngine(a, sd, device="cuda:0", dtype="bf16", max_seqs=1, max_positions=256, use_graph=use_graph)
    assert eng.options().endswith("|w13=5")
    app = _applicable(a.d_model)
    for layer in eng.w13_stats():
        for bit, m in zip((1, 4), eng.W13_MATRICES):
            assert layer[m] == {"state": "packed" if app & bit else "not_applicable", "refused_fragments": 0}, (m, layer)
    eng.set_option("w13", 0)
    c0 = eng.launch_counts()
    want = _logits(eng, prompt, toks)
    c_off = _delta(eng.launch_counts(), c0)
    assert c_off["w13"] == 0 and c_off["row_gemm_fr1"] > 0, c_off
    assert np.isfinite(want[np.abs(want) < 1e3]).all() and np.abs(want).max() > 0
    for v in (5, 1, 4):
        eng.set_option("w13", v)
        assert eng.options().endswith(f"|w13={v}")
        c0 = eng.launch_counts()
        got = _logits(eng, prompt, toks)
        c = _delta(eng.launch_counts(), c0)
        assert np.array_equal(got, want), (v, float(np.abs(got - want).max()))
        assert (c["w13"] > 0) == bool(v & app), (v, c)
        # The planes launches keep counting in their bf16 twins' slots, and once more in `w13`.  Every decode step of a call launches
        # the same kernels (eager: counted per step, and the loop launches steps in batches while the host runs ahead, so the totals
        # of two calls differ; captured: counted once, at capture), one paired QKV projection and one FFN down-projection per layer:
        assert c["row_gemm_fr1"] > 0 and c["row_gemm_fr1"] % 2 == 0 and c["rows_gemm"] > 0, (v, c)
        assert c["w13"] == c["row_gemm_fr1"] // 2 * bin(v & app).count("1"), (v, c)


@pytest.mark.parametrize("dtype,preset", [("bf16", "tiny"), ("fp32", "tiny128")])
def test_w13_not_applicable_narrow_width_and_fp32(dtype, preset):
    """d = 256 (no wave share of four fragments) and an fp32 engine: the option is accepted, nothing is packed, nothing changes."""
    from voicecraft_amd import synth
    from voicecraft_amd.engine import VoiceCraftEngine
    a = synth.make_args(preset)
    sd = synth.make_state_dict(a, seed=4)
    prompt = synth.random_prompt(a, 6, 20, seed=3)
    toks = _model("tiny128")[3]
    eng = VoiceCraftEngine(a, sd, device="cuda:0", dtype=dtype, max_seqs=1, max_positions=256)
    assert all(v["state"] == "not_applicable" for layer in eng.w13_stats() for v in layer.values())
    for bad in (2, 7, 8, -1):               # not a mask of 1 | 4: VC_EINVAL (an AssertionError, as for every bad input), the state stays
        with pytest.raises(AssertionError):
            eng.set_option("w13", bad)
        assert eng.options().endswith("|w13=5")
    out = {}
    for v in (0, 5):
        eng.set_option("w13", v)
        c0 = eng.launch_counts()
        out[v] = _logits(eng, prompt, toks)
        assert _delta(eng.launch_counts(), c0)["w13"] == 0
    assert np.array_equal(out[0], out[5])


def _sprinkle(w, gamma=None):
    """Zeros, -0.0, a denormal and both ends of a 30-binade window into the fragments at the matrix's corner (rows 0..15 x columns
    0..63 = fragments (0, 0) and (1, 0) of the 8 x 64 layout) and into two further down; the LayerNorm weight of the
    touched columns is set to 1 so that the folded matrix holds exactly these values."""
    for r0, c0 in ((0, 0), (32, 128)):
        blk = w[r0:r0 + 16, c0:c0 + 64]
        blk.uniform_(0.01, 0.03)                        # hi7 = 60
        blk[0, 0] = 0.0
        blk[1, 1] = -0.0
        blk[2, 2] = 1e-39
        blk[3, 3] = -1e-39
        blk[4, 4] = 1.5                                 # hi7 = 63: the top of the window
        blk[5, 5] = -2.0 ** -29                         # hi7 = 49: its bottom (15 steps)
        blk[9, 17] = 1.0
        blk[10, 18] = 2.0 ** -28
        if gamma is not None:
            gamma[c0:c0 + 64] = 1.0


def _edited(preset):
    a, sd, prompt, toks = _model(preset)
    sd = {k: v.clone() for k, v in sd.items()}
    for l in range(a.num_decoder_layers):
        p = f"decoder.layers.{l}."
        _sprinkle(sd[p + "linear2.weight"])
        _sprinkle(sd[p + "self_attn.in_proj_weight"], sd[p + "norm1.weight"])
    return a, sd, prompt, toks


@pytest.mark.parametrize("preset", ["tiny128", "giga330M"])
def test_w13_edited_checkpoint_zero_code_and_window_ends_stay_packed(preset):
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sd, prompt, toks = _edited(preset)
    eng = VoiceCraftEngine(a, sd, device="cuda:0", dtype="bf16", max_seqs=1, max_positions=256)
    app = _applicable(a.d_model)
    for layer in eng.w13_stats():
        for bit, m in zip((1, 4), eng.W13_MATRICES):
            assert layer[m] == {"state": "packed" if app & bit else "not_applicable", "refused_fragments": 0}, (m, layer)
    eng.set_option("w13", 0)
    want = _logits(eng, prompt, toks)
    eng.set_option("w13", 5)
    c0 = eng.launch_counts()
    got = _logits(eng, prompt, toks)
    assert _delta(eng.launch_counts(), c0)["w13"] > 0
    assert np.array_equal(got, want), float(np.abs(got - want).max())


@pytest.mark.parametrize("preset", ["tiny128", "giga330M"])
def test_w13_refused_matrix_keeps_its_bf16_launch(preset):
    """1.0 next to 1e-12 in ONE fragment of layer 1's FFN down-projection: the statistics show exactly that matrix refused (one
    fragment), its launches stay on the bf16 kernel, every other matrix stays packed, and the results are those of option off."""
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sd, prompt, toks = _edited(preset)
    w = sd["decoder.layers.1.linear2.weight"]
    w[40, 200] = 1.0
    w[41, 201] = 1e-12
    eng = VoiceCraftEngine(a, sd, device="cuda:0", dtype="bf16", max_seqs=1, max_positions=256, use_graph=False)
    L = a.num_decoder_layers
    qkv = bool(_applicable(a.d_model) & 4)
    st = eng.w13_stats()
    for l in range(L):
        assert st[l]["qkv"] == {"state": "packed" if qkv else "not_applicable", "refused_fragments": 0}, st[l]
        assert st[l]["ffn_down"] == ({"state": "refused", "refused_fragments": 1} if l == 1 else {"state": "packed", "refused_fragments": 0}), st[l]
    eng.set_option("w13", 0)
    want = _logits(eng, prompt, toks)
    # eager: every launch of the call is counted; each step launches one FFN down-projection and one paired QKV projection per layer
    for v, per_step in ((1, L - 1), (4, L if qkv else 0), (5, L - 1 + (L if qkv else 0))):
        eng.set_option("w13", v)
        c0 = eng.launch_counts()
        got = _logits(eng, prompt, toks)
        c = _delta(eng.launch_counts(), c0)
        n_down = c["row_gemm_fr1"] // 2
        assert n_down > 0 and n_down % L == 0 and c["w13"] == n_down // L * per_step, (v, c)
        assert np.array_equal(got, want), v
