"""The 8-bit weight grid of option `w8` (voicecraft_amd/csrc/vc_w8.h, voicecraft_amd/quant.py), without a GPU.

* The quantiser: its output lies on the grid in every 8 x 64 block (checked by a numpy decoder written here, which shares nothing with
  quant.py or the header), a second pass changes nothing, and the error is the grid's own: half an ulp of a 3-bit mantissa (2^-4
  relative) for every value in a block's normal range, half a denormal step (2^(s - 10) absolute) below it.  Both bounds are
  derivations, not measurements.
  The normal range is |v| >= 2^(s - 6) with s the block's shift.  s = emax - 8 (emax: the binade of the block's largest input), so the
  range reaches 2^-14 of that binade, for every block whose largest value is at most 464 . 2^(emax - 8).  Above 464 - past the midpoint
  between 448 and E4M3's NaN code 480 - NO 8-bit shift keeps 2^-4 for the block's largest value AND for its binade emax - 14 (448 and
  512 are both further than 1/16 from 480): quant.py takes s = emax - 7 there, which keeps 2^-4 for the large values and gives the
  lowest binade up to the denormal step.  The test pins exactly that: s = emax - 8 unless the block maximum is above 464 . 2^(emax - 8).
* tools/w8_check.cpp - the header's encode / decode under -fsanitize=address,undefined: all 254 non-NaN codes at both ends of the
  allowed shifts, and the refusals (an off-grid value, a value that needs the NaN code, a fragment whose shift would leave the normal
  bf16 range)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFT_MIN, SHIFT_MAX = -117, 119


# ---- an independent statement of the grid: E4M3 (e4m3fn) magnitudes by enumeration, block membership by search over the shifts
def e4m3_magnitudes() -> np.ndarray:
    """The 127 magnitudes of the non-NaN codes (0 included), as float64."""
    out = []
    for code in range(0x7f):                     # 0x7f = S.1111.111 is the NaN code
        e, m = code >> 3, code & 7
        out.append(m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
    return np.array(sorted(set(out)))


E4M3 = e4m3_magnitudes()


def is_normal_bf16_or_zero(v: np.ndarray) -> np.ndarray:
    a = np.abs(v.astype(np.float64))
    f32 = v.astype(np.float32)
    is_bf16 = (f32.view(np.uint32) & 0xffff) == 0
    return is_bf16 & ((a == 0) | ((a >= 2.0 ** -126) & (a < 2.0 ** 128)))


def block_grid_shift(block: np.ndarray):
    """The smallest shift s of the allowed range with every value of the block = q . 2^s, q a non-NaN E4M3 number; None if there is none."""
    a = np.abs(block.astype(np.float64)).ravel()
    nz = a[a > 0]
    if nz.size == 0:
        return 0
    emax = int(np.floor(np.log2(nz.max())))
    for s in range(max(emax - 9, SHIFT_MIN), min(emax + 10, SHIFT_MAX) + 1):
        if np.isin(nz / 2.0 ** s, E4M3).all():
            return s
    return None


def blocks_of(w: np.ndarray):
    n, k = w.shape
    assert n % 8 == 0 and k % 64 == 0
    for r in range(0, n, 8):
        for c in range(0, k, 64):
            yield (r, c), w[r:r + 8, c:c + 64]


def assert_on_grid(w: torch.Tensor) -> dict:
    w = w.numpy()
    assert np.isfinite(w).all()
    assert is_normal_bf16_or_zero(w).all(), "a grid value is a normal bf16 number or +-0"
    shifts = {}
    for rc, blk in blocks_of(w):
        s = block_grid_shift(blk)
        assert s is not None, f"block {rc} is off the grid"
        shifts[rc] = s
    return shifts


def spread_matrix() -> torch.Tensor:
    """64 x 256 (8 x 4 blocks), bf16-valued: magnitudes over 30 binades inside every block, zeros, -0.0, and per block a largest value
    chosen against the top of the grid - 450 .. 510 . 2^s0, on both sides of 464 and of the NaN code 480 - and plain random maxima."""
    g = torch.Generator().manual_seed(5)
    w = torch.randn(64, 256, generator=g) * torch.exp2(torch.randint(-30, 1, (64, 256), generator=g).float())
    w = w.bfloat16().float()
    tops = [450.0, 464.0, 466.0, 470.0, 478.0, 480.0, 482.0, 496.0, 500.0, 510.0, 448.0, 256.0, 254.0, 462.0, 476.0, 484.0]      # bf16 numbers
    for i, ((r, c), _) in enumerate(blocks_of(w.numpy())):
        blk = w[r:r + 8, c:c + 64]
        blk[0, 0] = 0.0
        blk[1, 1] = -0.0
        blk[2, 2:6] = 0.0
        if i < len(tops):
            s0 = -12 + 3 * i                                    # the block's binade moves too, 45 binades over the blocks
            blk.clamp_(-255.0 * 2.0 ** s0, 255.0 * 2.0 ** s0)
            blk[3, 3] = tops[i] * 2.0 ** s0                     # the largest value: emax - 8 = s0
            blk[4, 4] = -tops[i] * 2.0 ** s0
            blk[5, 5] = 2.0 ** (s0 - 6)                         # the bottom of the normal range at s0
            blk[6, 6] = 1.5 * 2.0 ** (s0 - 6)
            blk[7, 7] = 2.0 ** (s0 - 9)                         # the smallest denormal at s0
            blk[7, 8] = 0.4 * 2.0 ** (s0 - 9)                   # below half of it: becomes 0
    w = w.bfloat16().float()
    assert bool((w.abs() > 0).any()) and bool(((w == 0) & torch.signbit(w)).any())
    return w


def test_quantiser_grid_idempotence_and_error_bounds():
    from voicecraft_amd import quant
    w = spread_matrix()
    q = quant.quantize_image(w)
    assert q.dtype == torch.float32 and q.shape == w.shape and bool(torch.isfinite(q).all())
    shifts = assert_on_grid(q)
    assert torch.equal(quant.quantize_image(q).view(torch.int32), q.view(torch.int32)), "a second pass changes nothing (signs of zeros included)"
    wn, qn = w.numpy().astype(np.float64), q.numpy().astype(np.float64)
    n_norm = n_sub = n_shift_up = 0
    for (r, c), blk in blocks_of(wn):
        amax = np.abs(blk).max()
        emax = int(np.floor(np.log2(amax)))
        # the quantiser's shift, recovered from its documented rule; the decoder's smallest shift can only be lower or equal
        up = amax > 464.0 * 2.0 ** (emax - 8)
        s = emax - 8 + (1 if up else 0)
        n_shift_up += int(up)
        assert shifts[(r, c)] <= s, ((r, c), shifts[(r, c)], s)
        out = qn[r:r + 8, c:c + 64]
        assert np.abs(out).max() <= 448.0 * 2.0 ** s
        normal = np.abs(blk) >= 2.0 ** (s - 6)                  # = 2^-14 of the block maximum's binade when s = emax - 8
        rel = np.abs(out[normal] - blk[normal]) / np.abs(blk[normal])
        assert rel.max() <= 2.0 ** -4, ((r, c), float(rel.max()))
        assert (np.abs(out[~normal] - blk[~normal]) <= 2.0 ** (s - 10)).all(), (r, c)
        assert (np.signbit(out) == np.signbit(blk)).all(), "signs stay, those of zeros too"
        n_norm += int(normal.sum()); n_sub += int((~normal).sum())
    assert n_norm > 4000 and n_sub > 4000 and n_shift_up >= 10, (n_norm, n_sub, n_shift_up)
    # rounding is to nearest EVEN: 2.5, 3.5 denormal steps -> 2, 4; 17, 19 sixteenths of 256 -> 256, 320 (mantissa steps of 32)
    t = torch.zeros(8, 64)
    t[0, 0] = 448.0
    t[0, 1:5] = torch.tensor([2.5, 3.5, -2.5, -3.5]) * 2.0 ** -9
    t[0, 5:9] = torch.tensor([272.0, 304.0, -272.0, -304.0])
    got = quant.quantize_image(t)[0, 1:9]
    assert got.tolist() == [2 * 2.0 ** -9, 4 * 2.0 ** -9, -2 * 2.0 ** -9, -4 * 2.0 ** -9, 256.0, 320.0, -256.0, -320.0]


def test_quantiser_tiny_blocks_and_shift_limits():
    """Blocks below 2^-109 keep the smallest shift (every result a normal bf16 number or 0), and the largest bf16 binade still fits."""
    from voicecraft_amd import quant
    w = torch.zeros(16, 64)
    w[:8] = (torch.randn(8, 64, generator=torch.Generator().manual_seed(1)) * 2.0 ** -118).bfloat16().float()
    w[8:] = (torch.randn(8, 64, generator=torch.Generator().manual_seed(2)).clamp(-3, 3) * 2.0 ** 125).bfloat16().float()
    q = quant.quantize_image(w)
    shifts = assert_on_grid(q)
    assert shifts[(0, 0)] == SHIFT_MIN and shifts[(8, 0)] <= SHIFT_MAX
    assert torch.equal(quant.quantize_image(q), q)


@pytest.mark.parametrize("seed", [0, 1])
def test_fold_assertion_holds_with_zero_and_negative_layernorm_weights(seed):
    """in_proj_weight: the grid holds bf16(W . gamma); the function returns Q / gamma, whose fold reproduces Q element by element."""
    from voicecraft_amd import quant
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(48, 128, generator=g) * 0.05
    gamma = 1.0 + 0.3 * torch.randn(128, generator=g)
    gamma[3] = 0.0
    gamma[64:70] = 0.0
    gamma[10] = -0.7
    gamma[100:110] *= -1.0
    gamma[20] = 1e-3
    gamma[21] = 37.0
    out = quant.quantize_matrix(w, gamma)                        # asserts the fold inside
    img = (out * gamma[None, :]).bfloat16().float()              # the engine's image: fp32 product, rounded to nearest even
    assert_on_grid(img)
    dead = gamma == 0
    assert torch.equal(out[:, dead], w[:, dead]), "columns with gamma = 0 are left alone"
    assert not torch.equal(out[:, ~dead], w[:, ~dead])
    assert torch.equal(quant.quantize_matrix(out, gamma), out), "idempotent"
    rel = ((img - (w * gamma[None, :]).bfloat16().float()).norm() / (w * gamma[None, :]).norm()).item()
    assert 0 < rel < 2.0 ** -4


def test_state_dict_differs_only_in_the_named_matrices():
    from voicecraft_amd import quant, synth
    a = synth.make_args("tiny128")
    sd = synth.make_state_dict(a, seed=0)
    before = {k: v.clone() for k, v in sd.items() if torch.is_tensor(v)}
    for matrices, suffixes in ((("ffn_down", "qkv"), ("linear2.weight", "self_attn.in_proj_weight")), (("ffn_down",), ("linear2.weight",))):
        out = quant.quantize_state_dict_w8(a, sd, matrices=matrices)
        assert set(out) == set(sd)
        changed = sorted(k for k, v in out.items() if torch.is_tensor(v) and not torch.equal(v, before[k]))
        want = sorted(f"decoder.layers.{l}.{s}" for l in range(a.num_decoder_layers) for s in suffixes)
        assert changed == want
        assert all(out[k].dtype == torch.float32 and out[k].data_ptr() != sd[k].data_ptr() for k in want)
    assert all(torch.equal(sd[k], v) for k, v in before.items()), "the input is not modified"
    for l in range(a.num_decoder_layers):
        p = f"decoder.layers.{l}."
        assert_on_grid(out[p + "linear2.weight"].bfloat16().float())
    full = quant.quantize_state_dict_w8(a, sd)
    for l in range(a.num_decoder_layers):
        p = f"decoder.layers.{l}."
        assert_on_grid((full[p + "self_attn.in_proj_weight"] * full[p + "norm1.weight"][None, :]).bfloat16().float())
    again = quant.quantize_state_dict_w8(a, full)
    assert all(torch.equal(again[k], full[k]) for k in full if torch.is_tensor(full[k]))
    with pytest.raises(AssertionError):
        quant.quantize_state_dict_w8(a, sd, matrices=("ffn_up",))


def test_header_round_trip_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "w8_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", str(exe), os.path.join(ROOT, "tools", "w8_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    word, frags, refused = r.stdout.split()
    assert word == "ok" and int(frags) > 10000 and int(refused) > 2000, r.stdout
