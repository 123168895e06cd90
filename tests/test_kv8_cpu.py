"""The 8-bit grid of option `kv8` (voicecraft_amd/csrc/vc_kv8.h, voicecraft_amd/quant.py kv8_*), without a GPU.

* quant.kv8_quantize_rows against the independent numpy statement of tests/kv8_cases.py: codes and shifts bit for bit, the shift rule at
  the 464 boundary, idempotence, and the grid's own error - half an ulp of a 3-bit mantissa (2^-4 relative) for every value in the row's
  normal range |v| >= 2^(s - 6) that the clamp at 448 . 2^s does not touch, half a denormal step (2^(s - 10) absolute) below it.  Both
  bounds are derivations.  (Above 448 . 2^s - reached only by a row maximum in (448, 464] . 2^s - the clamp costs at most 16 / 464.)
* vc_kv8_quantize_host - the header's integer encode, the code the device packer runs - bit-equal to the quantiser.
* tools/kv8_check.cpp: the header under -fsanitize=address,undefined.
* the test oracle's hook: with an identity round trip it is the plain oracle's cached path, with the real one it is not.
* vc_debug_attn8 refuses what it should before it touches the device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import kv8_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("hd", kc.HDS)
def test_quantiser_against_the_independent_grid(hd):
    from voicecraft_amd import quant
    rows = torch.cat([kc.special_rows(hd), kc.random_rows(hd, 512, seed=1)])
    codes, shift = quant.kv8_quantize_rows(rows)
    assert codes.dtype == torch.uint8 and codes.shape == rows.shape and shift.dtype == torch.int8 and shift.shape == rows.shape[:-1]
    want_c, want_s = kc.grid_quantize(rows.numpy())
    assert np.array_equal(shift.numpy(), want_s)
    assert np.array_equal(codes.numpy(), want_c), np.argwhere(codes.numpy() != want_c)[:5]
    assert not ((codes.numpy() & 0x7f) == 0x7f).any(), "the NaN code is never stored"
    assert int(shift.min()) >= kc.SHIFT_MIN and int(shift.max()) <= kc.SHIFT_MAX
    # the shift rule, on the rows built for it: amax = top . 2^s0 takes s0 up to 464, s0 + 1 above
    r = rows.numpy().astype(np.float64)
    amax = np.abs(r).max(axis=1)
    nz = amax > 0
    emax = np.floor(np.log2(amax[nz]))
    base = np.clip(emax - 8, kc.SHIFT_MIN, kc.SHIFT_MAX)
    up = amax[nz] * 2.0 ** -base > 464.0
    assert np.array_equal(shift.numpy()[nz], np.minimum(base + up, kc.SHIFT_MAX)) and (shift.numpy()[~nz] == 0).all()
    assert up.sum() >= 10 and (~up).sum() >= 10
    for top, bump in ((448.0, 0), (464.0, 0), (kc.next_bf16_up(464.0), 1)):
        t = torch.zeros(1, hd)
        t[0, 0] = top * 2.0 ** -3
        assert int(quant.kv8_quantize_rows(t)[1]) == -3 + bump, top
    # dequantised values: bf16 numbers, the documented error, signs kept (those of zeros too), a second pass changes nothing
    back = quant.kv8_dequantize(codes, shift)
    assert torch.equal(back, back.bfloat16().float()) and bool(torch.isfinite(back).all())
    assert np.array_equal(back.numpy().astype(np.float64), kc.grid_values(want_c, want_s))
    assert torch.equal(quant.kv8_roundtrip(rows), back)
    c2, s2 = quant.kv8_quantize_rows(back)
    assert torch.equal(c2, codes) and torch.equal(s2, shift), "idempotent"
    assert np.array_equal(np.signbit(back.numpy()), np.signbit(rows.numpy()))
    s = shift.numpy().astype(np.float64)[:, None]
    b = back.numpy().astype(np.float64)
    normal = (np.abs(r) >= 2.0 ** (s - 6)) & (np.abs(r) <= 448.0 * 2.0 ** s)
    rel = np.abs(b - r)[normal] / np.abs(r)[normal]
    assert rel.max() <= 2.0 ** -4, float(rel.max())
    below = np.abs(r) < 2.0 ** (s - 6)
    assert (np.abs(b - r)[below] <= np.broadcast_to(2.0 ** (s - 10), r.shape)[below]).all()
    over = np.abs(r) > 448.0 * 2.0 ** s
    assert (np.abs(b[over]) == np.broadcast_to(448.0 * 2.0 ** s, r.shape)[over]).all() and over.sum() >= 2
    assert normal.sum() > 10000 and below.sum() > 1000
    # ties go to the even code
    t = torch.zeros(1, hd)
    t[0, 0] = 448.0
    t[0, 1:5] = torch.tensor([2.5, 3.5, -2.5, -3.5]) * 2.0 ** -9
    t[0, 5:9] = torch.tensor([272.0, 304.0, -272.0, -304.0])
    assert quant.kv8_roundtrip(t)[0, 1:9].tolist() == [2 * 2.0 ** -9, 4 * 2.0 ** -9, -2 * 2.0 ** -9, -4 * 2.0 ** -9, 256.0, 320.0, -256.0, -320.0]


@pytest.mark.parametrize("hd", kc.HDS)
def test_host_encode_is_bit_equal_to_the_quantiser(hd):
    from voicecraft_amd import engine, quant
    rows = torch.cat([kc.special_rows(hd), kc.random_rows(hd, 4096, seed=2)])
    codes, shift = quant.kv8_quantize_rows(rows)
    got_c, got_s = engine.kv8_quantize_host(rows.bfloat16())
    assert torch.equal(got_s, shift), torch.nonzero(got_s != shift)[:5]
    assert torch.equal(got_c, codes), torch.nonzero(got_c != codes)[:5]
    lead = rows[:96].reshape(4, 24, hd)                                  # leading dimensions are kept
    c3, s3 = engine.kv8_quantize_host(lead.bfloat16())
    assert c3.shape == lead.shape and s3.shape == lead.shape[:-1] and torch.equal(c3.reshape(-1, hd), codes[:96])


def test_header_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "kv8_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", str(exe), os.path.join(ROOT, "tools", "kv8_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    word, rows, vals = r.stdout.split()
    assert word == "ok" and int(rows) > 1000 and int(vals) > 50000, r.stdout


def test_the_oracle_hook():
    """Identity round trip: the cached path of the plain oracle, exactly.  The quantiser's: something else, by about the grid's error."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    a = synth.make_args("tiny")
    sd = synth.make_state_dict(a, seed=0, fast=True)
    prompt = synth.random_prompt(a, 6, 12, seed=3)
    K = a.n_codebooks
    n = 6
    toks = np.random.RandomState(5).randint(0, a.audio_vocab_size, size=(n, K)).astype(np.int64)
    for j in range(K):
        toks[n - K + j, :j] = a.empty_token
        toks[n - K + j, j] = a.eos
    torch.set_num_threads(min(4, torch.get_num_threads()))
    plain = kc.cached_tts_logits(VoiceCraftOracle(a, sd), prompt, toks)
    seen = []

    def ident(t):
        seen.append(tuple(t.shape))
        return t

    same = kc.cached_tts_logits(kc.Kv8Oracle(a, sd, roundtrip=ident), prompt, toks)
    assert plain.shape == (n, K, a.audio_vocab_size + int(a.n_special)) and np.array_equal(same, plain)
    L = a.num_decoder_layers
    assert len(seen) == (n - 1) * L and all(s[0] == 2 and s[-1] == a.d_model // a.nhead for s in seen), "every cached step of every layer goes through the hook"
    assert [s[-2] for s in seen[::L]] == list(range(seen[0][-2], seen[0][-2] + n - 1)), "... with the whole past, one position more per step"
    real = kc.cached_tts_logits(kc.Kv8Oracle(a, sd), prompt, toks)
    assert np.array_equal(real[0], plain[0]), "the first step reads no cache"
    d = np.abs(real[1:] - plain[1:]).max()
    assert 0 < d < 0.5 * np.abs(plain).max(), d


def test_debug_attn8_refuses_without_touching_the_device():
    from voicecraft_amd import _lib
    lib = _lib.load()

    def call(**kw):
        base = dict(q=16, kcache=32, vcache=48, row_seq=4, row_pos=8, n_active=12, share_len=20, att_o=64, att_ml=80, x_out=None,
                    dtype=1, H=2, hd=64, S_max=128, rows=3, nsplit=4, nt=0, fast=1, part16=0)
        top = dict(kcache8=96, vcache8=112, kvshift8=130, rps=1, pack=0)
        for k, v in kw.items():
            (top if k in top else base)[k] = v
        return lib.vc_debug_attn8(C.byref(_lib.DebugAttn8Args(base=_lib.DebugAttnArgs(**base), **top)), None)

    bad = [dict(dtype=0), dict(dtype=2), dict(rps=0), dict(rps=-1), dict(hd=48), dict(hd=256), dict(nsplit=0), dict(nsplit=9), dict(rows=0),
           dict(H=0), dict(S_max=0), dict(x_out=96, nsplit=2), dict(x_out=96, nsplit=1, part16=1), dict(q=None), dict(q=20),
           dict(kcache=None), dict(vcache=None), dict(kcache=40), dict(kcache8=None), dict(vcache8=None), dict(kvshift8=None),
           dict(kcache8=100), dict(vcache8=120), dict(kvshift8=131), dict(row_seq=None), dict(row_pos=None), dict(n_active=None),
           dict(share_len=None), dict(att_o=None), dict(att_ml=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
    for kw in (dict(dtype=0), dict(rps=0), dict(hd=48), dict(kcache=None), dict(kcache8=None), dict(kcache8=100), dict(kvshift8=None),
               dict(kvshift8=131), dict(row_pos=None), dict(n_active=None), dict(rows=0)):
        assert call(pack=1, **kw) == -1, kw
    assert lib.vc_debug_attn8(None, None) == -1
    assert C.sizeof(_lib.DebugAttn8Args) == 152 and _lib.DebugAttn8Args.kcache8.offset == 120 and _lib.DebugAttn8Args.pack.offset == 148
    assert lib.vc_kv8_quantize_host(None, 1, 64, None, None) == -1
