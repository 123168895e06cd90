"""-m gpu: option `w8q` - on an engine created with `w8=` and `w8_qkv_rows=True`, the passes of finished rows whose QKV projection
reads the 12-channel image (9..16 rows; 7 and 8 at d = 2048; with `qkv_p8` below 2 the lower ones too) stream it, for layers 1.., from
the E4M3 pairs of that image (rows_gemm_qkvq_w8_k: the text of rows_gemm_k with the pairs as the weight source,
csrc/vc_gemm_rows_body.h).  The bytes decode to the same bf16 MFMA operands and everything else is the image kernel's text, so every
result is BIT-identical to `w8q = 0`: the tests compare with np.array_equal, eager and captured, at every width with a form (tiny128: 4
k-tiles per wave; giga330M: 8; giga830M: 16), in each kernel form's row range (2..4, 5..8, 9..16), with inactive rows, through a decode
session, next to the other w8 forms and kv8, and with a refused layer.  Value 12 (bit 8) takes the form whatever the measured win table
says, so the kernel is always reached.  The one tolerance is the project's bf16 bar against the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_w8_qkv_rows_cpu import KTW, ROWS_WIN, image12

pytestmark = pytest.mark.gpu

N_STEPS = 12
LAYERS = 2
OFF_GRID = (1.0 + 2.0 ** -7) * 2.0 ** -6          # eight significant bits: on no E4M3 grid (tests/test_gpu_w8.py)
PRESETS = ("tiny128", "giga330M", "giga830M")
PACKED = {"state": "packed", "refused_pairs": 0}
NOT_APPLICABLE = {"state": "not_applicable", "refused_pairs": 0}
# slots the eager loop (which launches steps ahead of the ones it takes, a number that depends on the host's timing) cannot move
FIXED_SLOTS = ("w8", "w13", "w8_wide", "w8_up", "row_gemm_fr1", "wd")


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


@functools.lru_cache(maxsize=None)
def _model(preset, live=False):
    """(args, the synthetic state dict with THREE matrices on the w8 grid, 20 prompts of different shapes): computed once, never
    modified.  live: terminators can be sampled (the recipe of tests/test_gpu_session.py), so that free-running calls end by themselves."""
    from voicecraft_amd import quant, synth
    a = synth.make_args(preset, num_decoder_layers=LAYERS)
    sd = synth.make_state_dict(a, seed=4, fast=True, mute_eos=False, boost=[(0, 2051, 0.45)]) if live else synth.make_state_dict(a, seed=0, fast=True)
    prompts = tuple(synth.random_prompt(a, 4 + (u % 5), 9 + 3 * (u % 7), seed=700 + u) for u in range(20))
    return a, quant.quantize_state_dict_w8(a, sd, ffn_up=True), prompts


def _forced(a, rows, ends=None):
    """[N_STEPS][rows][K] forced tokens; row u ends with step ends[u] (default: the last), by the staggered end of a span
    (voicecraft.py:1057-1066): the call ends with its forced steps."""
    K = a.n_codebooks
    toks = np.random.RandomState(17).randint(0, a.audio_vocab_size, size=(N_STEPS, rows, K)).astype(np.int64)
    for u in range(rows):
        n = N_STEPS if ends is None else ends[u]
        for j in range(K):
            toks[n - K + j, u, :j] = a.empty_token
            toks[n - K + j, u, j] = a.eos
    return toks


def _engine(a, sd, rows, w8="as_is", w8_qkv_rows=True, dtype="bf16", cls=None, use_graph=True, **kw):
    from voicecraft_amd.engine import VoiceCraftEngine
    if w8 is not None:
        kw["w8"] = w8
    return (cls or VoiceCraftEngine)(a, sd, device="cuda:0", dtype=dtype, max_seqs=rows, max_positions=256, use_graph=use_graph,
                                     w8_qkv_rows=w8_qkv_rows, **kw)


def _multi(eng, prompts, rows, forced):
    outs, lg = eng.inference_tts_multi([p[0][0] for p in prompts[:rows]], [p[2][0] for p in prompts[:rows]], top_k=1, stop_repetition=3,
                                       _forced=forced, _logit_steps=N_STEPS)
    return [o[0].cpu().numpy() for o in outs], lg.cpu().numpy()


def _plan(eng, a, mask, rows):
    """vc_debug_w8q_plan for the engine's model shape (default options): (the form is taken, k-tiles per wave)"""
    from test_w8_rows_cpu import cfg
    out = (C.c_int32 * 2)()
    c = cfg(a.d_model, a.nhead)
    assert eng.lib.vc_debug_w8q_plan(C.byref(c), mask, rows, out) == 0
    return out[0], out[1]


def _passes_fr(c):
    """Finished-row passes (2..16 rows: decode steps, and the prompts' last prefill rows) in a census difference.  A pass of 9..16 rows
    counts its out-projection and its FFN down-projection in rows_gemm_fr, one of 2..8 rows its out-projection there and its FFN
    down-projection in rows_gemm_frp: LAYERS of each per pass."""
    fr, frp = c["rows_gemm_fr"], c["rows_gemm_frp"]
    assert fr >= frp and (fr - frp) % 2 == 0 and (fr + frp) % (2 * LAYERS) == 0 and fr > 0, c
    return (fr + frp) // 2 // LAYERS


def _check_count(c, v, taken, min_steps):
    """c["w8_qkv_rows"] against the plan.  Every finished-row pass launches one QKV projection per layer >= 1 behind a centred copy:
    on the paired consumer (census slot rows_gemm_qp) at its row counts, else on the 12-channel image - the launches the form replaces,
    layer 0 never.  With bit 8 all of those take the form; value 4 follows the committed table, which also decides for the prefill
    passes' row counts (not known here)."""
    n = _passes_fr(c) * (LAYERS - 1) - c["rows_gemm_qp"]
    got = c["w8_qkv_rows"]
    if not (v & 4):
        assert got == 0, (v, c)
    elif v & 8:
        assert got == n, (v, c)
        assert not taken or got >= min_steps * (LAYERS - 1), (v, c)
    elif taken:
        assert min_steps * (LAYERS - 1) <= got <= n, (v, c)
    else:
        assert got <= n - min_steps * (LAYERS - 1), (v, c)


def _legs(preset, rows, qkv_p8=None):
    """Logits and results of values 0 / 8 (refused) / 4 / 12, eager and captured, with the census checks."""
    a, sdq, prompts = _model(preset)
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows)
    assert eng.options().endswith("|w8=5|w8q=4")
    st = eng.w8_stats()
    assert st[0]["qkv_rows"] == NOT_APPLICABLE and all(layer["qkv_rows"] == PACKED for layer in st[1:]), st
    if qkv_p8 is not None:
        eng.set_option("qkv_p8", qkv_p8)
    # the 12-channel launch serves these rows: past the paired consumer's row counts, or with the paired consumer off
    on_image = qkv_p8 is not None and qkv_p8 < 2 or rows > (6 if a.d_model >= 2048 else 8)
    assert on_image
    if qkv_p8 is None:
        assert _plan(eng, a, 12, rows) == (1, KTW[a.d_model])
    for use_graph in (False, True):
        eng.use_graph = use_graph
        ref = None
        for v in (0, 8, 4, 12):
            if v == 8:      # bit 8 alone is no value of the option: refused, and the leg runs as the first one did
                with pytest.raises(AssertionError):
                    eng.set_option("w8q", 8)
                assert eng.options().endswith("|w8=5|w8q=0")
            else:
                eng.set_option("w8q", v)
                assert eng.options().endswith(f"|w8=5|w8q={v}")
            taken = bool(v & 4) and (bool(v & 8) or rows in ROWS_WIN)
            if qkv_p8 is None and v != 8:
                assert _plan(eng, a, v, rows)[0] == int(taken)
            c0 = eng.launch_counts()
            res, lg = _multi(eng, prompts, rows, forced)
            c = _delta(eng.launch_counts(), c0)
            assert eng.last_steps == N_STEPS             # every row ends with the last forced step: the step width never changes
            if ref is None:
                ref = (res, lg, c)
                assert np.isfinite(lg[np.abs(lg) < 1e3]).all() and np.abs(lg).max() > 0
            assert np.array_equal(lg, ref[1]), (use_graph, v, float(np.abs(lg - ref[1]).max()))
            assert all(np.array_equal(r, w) for r, w in zip(res, ref[0]))
            if v == 8:      # the state of the first leg once more: captured, its graphs are replayed and the census sees no launch
                assert c["w8_qkv_rows"] == 0, c
                continue
            if not use_graph:
                assert _passes_fr(c) >= N_STEPS - 1, c
            _check_count(c, v, taken, (N_STEPS - 1) if not use_graph else 1)
            # the option moves no launch to another form and counts in no older slot
            for slot in c:
                if slot != "w8_qkv_rows" and (use_graph or slot in FIXED_SLOTS):
                    assert c[slot] == ref[2][slot], (slot, v, c, ref[2])


@pytest.mark.parametrize("preset,rows", [(p, r) for p in PRESETS for r in (9, 16)] + [("giga830M", 7), ("giga830M", 8)])
def test_w8q_logits_bit_identical_and_census(preset, rows):
    _legs(preset, rows)


@pytest.mark.parametrize("rows", (2, 4, 5, 8))
@pytest.mark.parametrize("preset", PRESETS)
def test_w8q_follows_the_image_launch_below_the_paired_consumer(preset, rows):
    """`qkv_p8 = 1`: the 12-channel launch serves 2..8 rows too - kernel forms (NTW, R2) = (1, false) and (2, false)."""
    _legs(preset, rows, qkv_p8=1)


@pytest.mark.parametrize("shrink", [1, 0])
def test_w8q_inactive_and_ragged_rows(shrink):
    """Row 0 ends six steps before the others: with shrink off its row stays in the step without a position, with shrink on the live
    rows move onto an 11-row step, which takes the same kernel form."""
    a, sdq, prompts = _model("giga830M")
    rows = 12
    forced = _forced(a, rows, ends=[N_STEPS - 6] + [N_STEPS] * (rows - 1))
    eng = _engine(a, sdq, rows)
    eng.set_option("shrink", shrink)
    out = {}
    for v in (0, 12):
        eng.set_option("w8q", v)
        c0 = eng.launch_counts()
        out[v] = _multi(eng, prompts, rows, forced)
        _check_count(_delta(eng.launch_counts(), c0), v, True, 1)
    (res0, lg0), (res1, lg1) = out[0], out[12]
    T = [p[2].shape[1] for p in prompts[:rows]]
    assert res0[0].shape[-1] - T[0] < res0[1].shape[-1] - T[1], [r.shape for r in res0]
    assert all(r0.shape == r1.shape and np.array_equal(r0, r1) for r0, r1 in zip(res0, res1))
    assert np.array_equal(lg0, lg1), float(np.abs(lg0 - lg1).max())


def test_w8q_session_widths_through_the_range():
    """18 seeded requests of different lengths through twelve slots, `w8r`, `w8m` and `w8ur` on in both legs: the step width moves
    through 9..12 while the queue refills the slots and through 8..2 when it drains."""
    a, sdq, prompts = _model("giga830M", live=True)
    got = {}
    for on in (False, True):
        eng = _engine(a, sdq, 12, w8_rows=True, w8_mid=True, w8_up_rows=True)
        assert eng.options().endswith("|w8=5|w8r=5|w8m=1|w8ur=2|w8q=4")
        eng.set_option("w8q", 12 if on else 0)
        c0 = eng.launch_counts()
        outs = eng.inference_tts_queue([p[0][0] for p in prompts[:18]], [p[2][0] for p in prompts[:18]], max_live=12,
                                       seeds=[100 + u for u in range(18)], top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3)
        c = _delta(eng.launch_counts(), c0)
        assert eng.last_session_stats["admitted"] == 18, eng.last_session_stats
        assert c["rows_gemm_fr"] > c["rows_gemm_frp"] > 0 and c["rows_gemm_qp"] > 0, c      # steps of 9..12 rows and of 2..8 rows both ran
        assert c["w8_mid"] > 0 and c["w8_rows"] > 0 and c["w8_up_rows"] > 0 and (c["w8_qkv_rows"] > 0) == on, c
        got[on] = [o[0].cpu().numpy() for o in outs]
        del eng
    lens = [r.shape[-1] - p[2].shape[1] for r, p in zip(got[False], prompts)]
    assert len(set(lens)) > 1, lens
    assert all(r0.shape == r1.shape and np.array_equal(r0, r1) for r0, r1 in zip(got[False], got[True]))


def test_w8q_next_to_the_wide_form_of_the_same_matrix():
    """A ragged batch of 20 on an engine with `w8_wide=True` too: rows 12..19 end six steps early, the step shrinks from 20 rows - QKV
    on the 16-channel pair planes through `w8w` - to 12, where `w8q` reads the 12-channel pairs of the same checkpoint."""
    a, sdq, prompts = _model("giga830M")
    rows = 20
    forced = _forced(a, rows, ends=[N_STEPS - 6 if u >= 12 else N_STEPS for u in range(rows)])
    eng = _engine(a, sdq, rows, w8_wide=True)
    assert eng.options().endswith("|w8=5|w8w=5|w8q=4")
    assert all(layer["qkv_wide"]["state"] == "packed" for layer in eng.w8_stats()), eng.w8_stats()
    eng.set_option("shrink", 1)
    out = {}
    for on in (False, True):
        eng.set_option("w8q", 12 if on else 0)
        c0 = eng.launch_counts()
        out[on] = _multi(eng, prompts, rows, forced)
        c = _delta(eng.launch_counts(), c0)
        assert c["wd"] > 0 and c["rows_gemm_fr"] > 0 and c["w8_wide"] > 0, c      # wide steps and 12-row steps both ran
        _check_count(c, 12 if on else 0, True, 1)
    (res0, lg0), (res1, lg1) = out[False], out[True]
    assert all(r0.shape == r1.shape and np.array_equal(r0, r1) for r0, r1 in zip(res0, res1))
    assert np.array_equal(lg0, lg1), float(np.abs(lg0 - lg1).max())


def test_w8q_next_to_kv8():
    a, sdq, prompts = _model("giga330M")
    rows = 12
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows, kv8=True)
    assert eng.options().endswith("|w8=5|w8q=4|kv8=1")
    out = {}
    for v in (0, 12):
        eng.set_option("w8q", v)
        c0 = eng.launch_counts()
        out[v] = _multi(eng, prompts, rows, forced)
        c = _delta(eng.launch_counts(), c0)
        assert c["kv8_attn"] > 0, c
        _check_count(c, v, True, 1)
    assert np.array_equal(out[0][1], out[12][1]) and all(np.array_equal(r0, r1) for r0, r1 in zip(out[0][0], out[12][0]))


def test_w8q_one_off_grid_value_keeps_its_layer_on_the_image():
    from voicecraft_amd import quant
    a, sdq, prompts = _model("giga330M")
    from voicecraft_amd import synth
    a3 = synth.make_args("giga330M", num_decoder_layers=3)
    sd3 = {k: v.clone() for k, v in sdq.items()}
    for k in list(sdq):      # a third layer (a copy of layer 1), so that one packed layer stays next to the refused one
        if k.startswith("decoder.layers.1."):
            sd3[k.replace("decoder.layers.1.", "decoder.layers.2.")] = sdq[k].clone()
    sd3["decoder.layers.1.self_attn.in_proj_weight"][9, 200] = OFF_GRID
    img = quant.fold(sd3["decoder.layers.1.self_attn.in_proj_weight"], sd3["decoder.layers.1.norm1.weight"])
    assert quant.quantize_image(img)[9, 200] != img[9, 200]             # the folded value is off the grid too
    rows = 12
    forced = _forced(a3, rows)
    eng = _engine(a3, sd3, rows, use_graph=False)
    st = eng.w8_stats()
    assert st[0]["qkv_rows"] == NOT_APPLICABLE and st[2]["qkv_rows"] == PACKED, st
    assert st[1]["qkv_rows"]["state"] == "refused" and st[1]["qkv_rows"]["refused_pairs"] >= 1, st
    eng.set_option("w8q", 0)
    res0, want = _multi(eng, prompts, rows, forced)
    # eager: every launch is counted; the QKV projections of layers 0 and 1 stay on rows_gemm_k, layer 2's takes the form
    eng.set_option("w8q", 12)
    c0 = eng.launch_counts()
    res1, got = _multi(eng, prompts, rows, forced)
    c = _delta(eng.launch_counts(), c0)
    fr, frp = c["rows_gemm_fr"], c["rows_gemm_frp"]
    passes = (fr + frp) // 2 // 3
    assert passes >= N_STEPS - 1 and N_STEPS - 1 <= c["w8_qkv_rows"] <= passes, c
    assert np.array_equal(got, want) and all(np.array_equal(r0, r1) for r0, r1 in zip(res0, res1))


def test_w8q_against_the_oracle_on_the_quantised_checkpoint():
    """`w8="quantize"` with `w8_qkv_rows=True` quantises what `w8=` alone does; teacher-forced logits of a 12-row call meet the project's
    bf16 bar (per-step relative L2 <= 2e-2) against the oracle on that checkpoint for three of the rows, and equal a plain
    bf16 engine's on that checkpoint bit for bit."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from test_gpu_model import rel_l2
    from voicecraft_amd import quant, synth
    rows, utts = 12, (0, 5, 11)
    a, _, prompts = _model("tiny128")
    sd = synth.make_state_dict(a, seed=0, fast=True)
    forced = _forced(a, rows)
    eng = _engine(a, sd, rows, w8="quantize")
    two = quant.quantize_state_dict_w8(a, sd)
    assert all(torch.equal(eng.w8_state_dict[k], two[k]) for k in two if torch.is_tensor(two[k]))      # no new matrix is quantised
    assert all(layer["qkv_rows"] == PACKED for layer in eng.w8_stats()[1:])
    eng.set_option("w8q", 12)
    c0 = eng.launch_counts()
    _, got = _multi(eng, prompts, rows, forced)
    assert _delta(eng.launch_counts(), c0)["w8_qkv_rows"] > 0
    _, plain = _multi(_engine(a, eng.w8_state_dict, rows, w8=None, w8_qkv_rows=False), prompts, rows, forced)
    assert np.array_equal(got, plain)
    torch.set_num_threads(min(4, torch.get_num_threads()))
    orc = VoiceCraftOracle(a, eng.w8_state_dict)
    for u in utts:
        x, _, y = prompts[u]
        want = orc.tts_logits_for_trajectory(x, y, forced[:, u], steps=list(range(N_STEPS))).numpy()
        rel = float(rel_l2(got[:, u].reshape(want.shape), want).max())
        print(f"tiny128, {rows} rows, utterance {u}: w8q engine against the oracle on the quantised checkpoint: worst rel L2 {rel:.2e}")
        assert rel <= 2e-2, (u, rel)


def test_no_request_nothing_new_and_refusals():
    from test_w8_rows_cpu import cfg
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sdq, prompts = _model("tiny128")
    rows = 12
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows, w8="as_is", w8_qkv_rows=False, w8_mid=True)
    assert eng.options().endswith("|w8=5|w8m=1") and "w8q" not in eng.options()
    assert all("qkv_rows" not in layer for layer in eng.w8_stats())
    for v in (0, 4, 12):
        with pytest.raises(AssertionError):
            eng.set_option("w8q", v)
        assert eng.options().endswith("|w8=5|w8m=1")
    with pytest.raises(AssertionError):
        eng.debug_read("w8q_stats", (LAYERS, 2), torch.int32)
    c0 = eng.launch_counts()
    _multi(eng, prompts, rows, forced)
    c = _delta(eng.launch_counts(), c0)
    assert c["w8_qkv_rows"] == 0 and c["w8_mid"] > 0, c
    assert eng.lib.vc_request_w8_qkv_rows(eng._h, 4) == -2      # VC_ESTATE: the request comes before vc_finalize_weights
    assert eng.options().endswith("|w8=5|w8m=1")
    with pytest.raises(ValueError):
        _engine(a, sdq, rows, w8=None, w8_qkv_rows=True)
    with pytest.raises(AssertionError):                         # bf16 operands: an fp32 engine refuses as it does for `w8`
        _engine(a, sdq, rows, dtype="fp32")
    for bad in (0, 1, 2, 5, 12, -1):                            # not the mask 4: VC_EINVAL, an AssertionError as for every bad input
        bad_cls = type("BadMask", (VoiceCraftEngine,), {"W8_QKV_ROWS_MASK": bad})
        with pytest.raises(AssertionError):
            _engine(a, sdq, rows, cls=bad_cls)
    # the order of the requests, on a bare handle
    lib = eng.lib
    h = C.c_void_p()
    c_ = cfg(a.d_model, a.nhead)
    assert lib.vc_create(C.byref(c_), 0, C.byref(h)) == 0
    try:
        assert lib.vc_request_w8_qkv_rows(h, 4) == -2           # VC_ESTATE: after vc_request_w8 only
        assert lib.vc_request_w8(h, 5) == 0
        for bad in (0, 1, 2, 5, 8, 12, -1):
            assert lib.vc_request_w8_qkv_rows(h, bad) == -1     # VC_EINVAL
        assert lib.vc_request_w8_mid(h, 4) == -1                # `w8m` keeps refusing bit 4
        assert lib.vc_request_w8_qkv_rows(h, 4) == 0
    finally:
        lib.vc_destroy(h)
    eng8 = _engine(a, sdq, rows)
    for bad in (1, 2, 5, 8, 13, 16, -1):
        with pytest.raises(AssertionError):
            eng8.set_option("w8q", bad)
        assert eng8.options().endswith("|w8=5|w8q=4")


def test_device_packer_equals_the_host_packer():
    """The planes and side bytes vc_finalize_weights packed on the GPU for layer 1 against vc_w8q_pack_host on the same folded image."""
    from test_w8_qkv_rows_cpu import pack_host
    from voicecraft_amd import quant
    a, sdq, _ = _model("giga330M")
    d = a.d_model
    eng = _engine(a, sdq, 12)
    img = quant.fold(sdq["decoder.layers.1.self_attn.in_proj_weight"], sdq["decoder.layers.1.norm1.weight"])
    pairs = image12(img.numpy())
    planes, side, refused = pack_host(pairs, d // 32)
    assert refused == 0
    n = pairs.shape[0]
    got_planes = eng.debug_read("w8q_planes_1", (n, 768), torch.uint8).cpu()
    got_side = eng.debug_read("w8q_side_1", (n, 2), torch.uint8).cpu()
    assert torch.equal(got_planes, planes) and torch.equal(got_side, side)
