"""`kv8="centred"` without a GPU (the contract: voicecraft_amd/csrc/vc_kv8.h, quant.py kv8c_*).

* vc_kv8c_quantize_host - the header's code, which the centred packer runs - bit-equal to quant.kv8c_quantize_rows and to the independent
  numpy grid of tests/kv8_cases.py applied to the centred rows, at centres of 0, 1 sigma and 20 sigma; with c = 0 the plain kv8 codes.
* invariance, float64: softmax over the scores the contract assembles equals softmax over the values each position stands for.
* quality - the test that fails without the mode: on trained_stats A the centred round trip costs at most 2 x what the bf16 cache costs.
* tools/kv8_check.cpp with the centred host row under -fsanitize=address,undefined.
* plan walk (vc_debug_kv8_plan, the function the engine's passes follow): centre then packer behind a centred engine's prefill passes,
  the centred attention form on its decode passes, a kv8=True engine's plan what it was.
* vc_debug_attn8c refuses what it should before it touches the device; an unknown kv8= string is refused."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import decode_attn_cases as dc
import kv8_cases as kc
import kv8c_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("hd", kc.HDS)
def test_host_entry_against_both_quantisers(hd):
    from voicecraft_amd import engine, quant
    rows = torch.cat([kc.special_rows(hd), kc.random_rows(hd, 1024, seed=4)])
    plain_c, plain_s = quant.kv8_quantize_rows(rows)
    moved = 0
    for mult, c in zip(cc.CENTRE_SIGMAS, cc.centres_for(rows, seed=hd)):
        # K rows = the test rows shifted by the centre: bf16 numbers again, finite
        k = kc.bf16(rows + c) if mult else rows                # (-0 + 0 would lose the special rows' signed zeros)
        keep = torch.isfinite(k).all(dim=-1)
        k = k[keep]
        assert keep.sum() >= rows.shape[0] - 2
        want_c, want_s = quant.kv8c_quantize_rows(k, c)
        got_c, got_s = engine.kv8c_quantize_host(k.bfloat16(), c.bfloat16())
        assert torch.equal(got_s, want_s), (mult, torch.nonzero(got_s != want_s)[:5])
        assert torch.equal(got_c, want_c), (mult, torch.nonzero(got_c != want_c)[:5])
        centred = (k - c).bfloat16().float()                               # the fp32 difference, rounded once to bf16
        grid_c, grid_s = kc.grid_quantize(centred.numpy())
        assert np.array_equal(got_s.numpy(), grid_s) and np.array_equal(got_c.numpy(), grid_c), mult
        assert not ((got_c.numpy() & 0x7f) == 0x7f).any(), "the NaN code is never stored"
        if mult == 0.0:
            assert torch.equal(got_c, plain_c[keep]) and torch.equal(got_s, plain_s[keep]), "c = 0: today's kv8 codes"
        else:
            moved += int((got_s != quant.kv8_quantize_rows(k)[1]).sum())      # against the uncentred grid of the same rows
        # what the cache then stands for: c + the grid's value, within the grid's half ulp of the SPREAD, not of the offset
        back = quant.kv8c_roundtrip(k, c)
        assert np.array_equal(back.numpy().astype(np.float64), kc.grid_values(grid_c, grid_s))
    assert moved > 100, "the centres must move rows to other shifts"
    lead = kc.bf16(rows[:96] + c).reshape(4, 24, hd)                       # leading dimensions are kept
    c3, s3 = engine.kv8c_quantize_host(lead.bfloat16(), c.bfloat16())
    assert c3.shape == lead.shape and s3.shape == lead.shape[:-1]
    from voicecraft_amd import _lib
    assert _lib.load().vc_kv8c_quantize_host(None, None, 1, 64, None, None) == -1


def test_centre_is_the_fp32_mean_rounded_once():
    from voicecraft_amd import quant
    g = torch.Generator().manual_seed(1)
    k = kc.bf16(torch.randn(3, 2, 37, 64, generator=g) + 5.0)
    c = quant.kv8c_centre(k)
    assert c.shape == (3, 2, 64) and torch.equal(c, c.bfloat16().float())
    m = k.double().mean(dim=-2)
    assert bool(((c.double() - m).abs() <= 2.0 ** -8 * m.abs() + 2.0 ** -20 * k.abs().max()).all())


@pytest.mark.parametrize("hd", kc.HDS)
def test_softmax_does_not_see_the_centre(hd):
    """Scores assembled as the contract says - 8-bit positions with + q . c, bf16 positions without - against the scores of the values
    each position stands for, in float64: equal up to float64 rounding, whatever the centre."""
    rng = np.random.RandomState(hd)
    scale = dc.kernel_scale(hd)
    for mult in (0.0, 1.0, 20.0):
        for S, lo in ((1, 0), (5, 2), (40, 37), (40, 40), (257, 255)):
            k = dc.bf16_exact(rng.randn(S, hd) + mult * rng.choice([-1.0, 1.0], size=hd))
            c = dc.bf16_exact(k[: max(lo, 1)].mean(axis=0)) if mult else np.zeros(hd, dtype=np.float32)
            q = dc.bf16_exact(rng.uniform(-1, 1, hd))
            sc, stands = cc.contract_scores(q, k, c, lo, scale)
            true = stands @ (q.astype(np.float64) * scale)
            assert np.allclose(sc, true, rtol=0, atol=1e-12 * (1 + np.abs(true).max()))
            w0, w1 = np.exp(sc - sc.max()), np.exp(true - true.max())
            assert np.allclose(w0 / w0.sum(), w1 / w1.sum(), rtol=0, atol=1e-12)
            if lo and mult:      # dropping q . c from the 8-bit positions alone is seen as soon as both kinds of positions are in the row
                wrong = sc.copy()
                wrong[:lo] -= (q.astype(np.float64) * scale) @ c.astype(np.float64)
                if lo < S:
                    w2 = np.exp(wrong - wrong.max())
                    assert np.abs(w2 / w2.sum() - w1 / w1.sum()).max() > 1e-6


@pytest.mark.parametrize("hd", kc.HDS)
def test_a_wrong_qc_exceeds_the_bar(hd):
    """The passes of tests/test_gpu_kv8c_attn.py (nsplit 1, 3, 8 of the edge table, and the shared-prefix table), the float64 reference
    perturbed: q . c left out of the 8-bit scores, added twice, taken from the other head, from another sequence.  Every launch has a row
    that each defect moves by at least SENS_MIN fp32-output bars; against the wider bf16-output bar the tables as a whole do."""
    es = cc.edge_entries(hd, nsplits=(1, 3, 8), defects=True) + cc.share_entries(hd, defects=True)
    for d in cc.DEFECTS:
        use = [e for e in es if not (d == "wrong_seq" and e["share"])]          # (under a shared prefix every sequence has sequence 0's centre)
        assert len(use) >= 12
        low = min(e["sens"][d][0] for e in use)
        assert low >= dc.SENS_MIN, (hd, d, low)
        assert max(e["sens"][d][1] for e in use) >= dc.SENS_MIN, (hd, d)
    c = es[0]["centre"].float()
    assert bool((c[0] != c[1]).any()) and bool((c[0, 0] != c[0, 1]).any()), "another offset per sequence and head"
    assert float(c.abs().min()) >= 10 * float(dc.content(hd, 64)[1].std()), "about 20 sigma on every channel"


QUALITY = {}


def _quality(preset):
    if preset not in QUALITY:
        torch.set_num_threads(min(4, torch.get_num_threads()))
        QUALITY[preset] = cc.quality_row(preset, "trained_stats_A")
    return QUALITY[preset]


@pytest.mark.parametrize("preset", ("tiny128", "tiny_h16"))
def test_centred_k_holds_under_peaked_attention(preset):
    """trained_stats A, tools/kv8_quality.py's method (fp32 oracle, 60 teacher-forced steps): the centred round trip's worst relative L2
    against the plain oracle is at most 2 x the bf16-only round trip's.  Measured: 1.33 x (tiny128), 1.25 x (tiny_h16); the plain kv8
    round trip stands at 10.8 x and is asserted to miss the bar, so that this test cannot pass on the uncentred grid.  The margin of 2
    covers the E4M3-versus-bf16 rounding of the spread that remains."""
    row = _quality(preset)
    print(row)
    bf16, kv8, kv8c = (row[t]["rel_l2_worst"] for t in ("bf16", "kv8", "kv8c"))
    assert row["steps"] == cc.STEPS
    assert kv8c <= 2.0 * bf16, (preset, kv8c, bf16)
    assert kv8 > 2.0 * bf16, "the uncentred grid meets the bar too: the setting is not peaked"


def test_header_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "kv8_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", str(exe), os.path.join(ROOT, "tools", "kv8_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe), "centred"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    word, rows, vals, mode, n_centred = r.stdout.split()
    assert word == "ok" and int(rows) > 2000 and int(vals) > 100000, r.stdout
    assert mode == "centred" and int(n_centred) >= 3 * 128 * 3 * 3, "the centred rows ran: three of four centres per row keep the difference finite at least"
    plain = subprocess.run([str(exe)], capture_output=True, text=True)
    assert plain.returncode == 0 and len(plain.stdout.split()) == 3 and int(plain.stdout.split()[1]) < int(rows), "without the argument: the plain rows only"


def test_plan_walk():
    """What the kv8 options add to a pass, from the host function that site_attn and run_pass follow (vc_engine.hip kv8_plan): per engine
    kind (request 0 none, 1 kv8=True, 2 centred), option value, pass kind (rps 0 = prefill, 1 and 3 = decode) and attention kernel."""
    from voicecraft_amd import _lib
    lib = _lib.load()
    PLAIN, E4M3, CENTRED = 0, 1, 2                  # VC_KV8_ATTN_*
    CENTRE, PACK, PACK_C = 1, 2, 3                  # VC_KV8_LAUNCH_*

    def plan(request, kv8, rps, rows_attn=1):
        out = (C.c_int32 * 4)(9, 9, 9, 9)
        assert lib.vc_debug_kv8_plan(request, kv8, rps, rows_attn, out) == 0
        return out[0], list(out[2:2 + out[1]]), list(out[2 + out[1]:])

    for rows_attn in (0, 1):                        # a prefill pass runs rows_attn_k (short prompts) or a tile kernel
        # a centred engine's prefill passes: bf16 attention, then centre -> packer, whatever the option's value
        for kv8 in (0, 1):
            assert plan(2, kv8, 0, rows_attn) == (PLAIN, [CENTRE, PACK_C], [])
            # a kv8=True engine's plan is what it was: bf16 attention on prefill, ONE packer launch behind every pass
            assert plan(1, kv8, 0, rows_attn) == (PLAIN, [PACK], [0])
            # no request: nothing at all
            for rps in (0, 1, 3):
                assert plan(0, kv8, rps, rows_attn) == (PLAIN, [], [0, 0])
    for rps in (1, 3):
        # decode passes: the centred form / the kv8 form, then the (centred) packer alone - no centre launch
        assert plan(2, 1, rps) == (CENTRED, [PACK_C], [0])
        assert plan(1, 1, rps) == (E4M3, [PACK], [0])
        # option kv8 = 0: the bf16 cache again; the engine goes on packing
        assert plan(2, 0, rps) == (PLAIN, [PACK_C], [0])
        assert plan(1, 0, rps) == (PLAIN, [PACK], [0])
        # (a decode pass never runs a tile kernel; if it did it would read the bf16 cache)
        assert plan(2, 1, rps, 0)[0] == PLAIN and plan(1, 1, rps, 0)[0] == PLAIN
    out = (C.c_int32 * 4)()
    assert lib.vc_debug_kv8_plan(3, 1, 1, 1, out) == -1 and lib.vc_debug_kv8_plan(-1, 1, 1, 1, out) == -1
    assert lib.vc_debug_kv8_plan(1, 1, -1, 1, out) == -1 and lib.vc_debug_kv8_plan(1, 1, 1, 1, None) == -1


def test_debug_attn8c_refuses_without_touching_the_device():
    from voicecraft_amd import _lib
    lib = _lib.load()

    def call(**kw):
        base = dict(q=16, kcache=32, vcache=48, row_seq=4, row_pos=8, n_active=12, share_len=20, att_o=64, att_ml=80, x_out=None,
                    dtype=1, H=2, hd=64, S_max=128, rows=3, nsplit=4, nt=0, fast=1, part16=0)
        mid = dict(kcache8=96, vcache8=112, kvshift8=130, rps=1, pack=0)
        top = dict(centre=144, n0=160, mode=0, n_seqs=4)
        for k, v in kw.items():
            (top if k in top else mid if k in mid else base)[k] = v
        a8 = _lib.DebugAttn8Args(base=_lib.DebugAttnArgs(**base), **mid)
        return lib.vc_debug_attn8c(C.byref(_lib.DebugAttn8cArgs(base8=a8, **top)), None)

    every = [dict(mode=-1), dict(mode=3), dict(centre=None), dict(centre=150), dict(dtype=0), dict(hd=48), dict(H=0), dict(S_max=0), dict(rows=0),
             dict(kcache=None), dict(kcache=40), dict(row_seq=None), dict(row_pos=None), dict(n_active=None)]
    for mode in (0, 1, 2):
        for kw in every:
            assert call(**{"mode": mode, **kw}) == -1, (mode, kw)
    for mode in (0, 1):
        for kw in (dict(rps=0), dict(vcache=None), dict(kcache8=None), dict(vcache8=None), dict(kvshift8=None), dict(kcache8=100),
                   dict(vcache8=120), dict(kvshift8=131)):
            assert call(mode=mode, **kw) == -1, (mode, kw)
    for kw in (dict(nsplit=0), dict(nsplit=9), dict(q=None), dict(q=20), dict(share_len=None), dict(att_o=None), dict(att_ml=None),
               dict(x_out=96, nsplit=2), dict(x_out=96, nsplit=1, part16=1)):
        assert call(mode=0, **kw) == -1, kw
    for kw in (dict(n0=None), dict(n_seqs=0), dict(n_seqs=65), dict(share_len=None), dict(rows=2049)):
        assert call(mode=2, **kw) == -1, kw
    assert lib.vc_debug_attn8c(None, None) == -1
    assert C.sizeof(_lib.DebugAttn8cArgs) == 176 and _lib.DebugAttn8cArgs.centre.offset == 152 and _lib.DebugAttn8cArgs.mode.offset == 168
    assert C.sizeof(_lib.DebugAttn8Args) == 152, "vc_debug_attn8_args is what it was"


def test_an_unknown_kv8_string_is_refused():
    from voicecraft_amd import synth
    from voicecraft_amd.engine import VoiceCraftEngine
    for bad in ("centered", "int8", "True"):
        with pytest.raises(ValueError, match="centred"):
            VoiceCraftEngine(synth.make_args("tiny"), {}, device="cuda:0", kv8=bad)
