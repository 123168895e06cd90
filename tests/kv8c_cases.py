"""`kv8="centred"` (centred K on the E4M3 copy of the K / V cache; the contract is in voicecraft_amd/csrc/vc_kv8.h and quant.py): what the
CPU and the GPU tests share.  No GPU here.  Builds on tests/kv8_cases.py and tests/decode_attn_cases.py and changes neither.

* centres of 0, 1 sigma and 20 sigma for the rows the quantiser is held to;
* the test oracle: Kv8Oracle whose cached K rows are read as c + kv8c_roundtrip(k, c), c the centre of the prompt's rows per layer and
  head (the rows of the first cached step's past: the prefill pass that wrote position 0), V through the plain kv8 round trip;
* the float64 score assembly of the contract, for the invariance check;
* the quality measurement (60 teacher-forced steps against the plain fp32 oracle): quality_row is what tools/kv8_quality.py prints and what
  the CPU quality test asserts on;
* the kernel-level offsets: about 20 sigma per channel, another one per head and sequence."""
from __future__ import annotations

import numpy as np
import torch

import decode_attn_cases as dc
import kv8_cases as kc

STEPS = 60
KNOBS = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=3)
CENTRE_SIGMAS = (0.0, 1.0, 20.0)


def centres_for(rows: torch.Tensor, seed: int = 0):
    """One bf16 centre per entry of CENTRE_SIGMAS for rows [n][hd]: sigma = the rows' standard deviation per channel (the median row
    scale, so that one huge special row does not set it), signs at random."""
    g = torch.Generator().manual_seed(77 + seed)
    sigma = rows.abs().median(dim=0).values.clamp_min(2.0 ** -20)
    sign = torch.where(torch.rand(rows.shape[-1], generator=g) < 0.5, -1.0, 1.0)
    return [kc.bf16(m * sigma * sign * (1.0 + 0.25 * torch.rand(rows.shape[-1], generator=g))) if m else torch.zeros(rows.shape[-1])
            for m in CENTRE_SIGMAS]               # (the centre of nothing is +0: k - (-0) would turn -0 into +0)


# ------------------------------------------------------------------------------------------------ the test oracle
class Kv8cOracle(kc.Kv8Oracle):
    """The kv8 test oracle with centred K.  `new_call()` before every call: the centre belongs to the prompt of the call."""

    def __init__(self, *a, **k):
        super().__init__(*a, roundtrip=lambda t: t, **k)
        self.centres = {}

    def new_call(self):
        self.centres = {}

    def _attn(self, l, x, mask, past_l):
        from voicecraft_amd import quant
        if past_l is not None:
            k16, v16 = past_l[0].bfloat16().float(), past_l[1].bfloat16().float()
            if l not in self.centres:                     # the first cached step: the past is the prompt, n0 rows
                self.centres[l] = (k16.shape[-2], quant.kv8c_centre(k16))
            n0, c = self.centres[l]
            assert k16.shape[-2] >= n0
            kq = c.unsqueeze(-2) + quant.kv8c_roundtrip(k16, c)
            past_l = torch.stack([kq, quant.kv8_roundtrip(v16)]).to(past_l.dtype)
        return kc.VoiceCraftOracle._attn(self, l, x, mask, past_l)


def centred_tts_logits(orc, prompt, toks):
    orc.new_call()
    return kc.cached_tts_logits(orc, prompt, toks)


def centred_edit_logits(orc, x, xl, y, spans, toks):
    orc.new_call()
    return kc.cached_edit_logits(orc, x, xl, y, spans, toks)


# ------------------------------------------------------------------------------------------------ quality (tools/kv8_quality.py's method)
def rel_l2(got, want):
    live = np.abs(want) < 1e3
    num = np.sqrt((((got - want) * live) ** 2).reshape(len(want), -1).sum(1))
    den = np.sqrt(((want * live) ** 2).reshape(len(want), -1).sum(1))
    return num / den


def quality_setup(preset, weights):
    """(args, state dict, prompt, the plain fp32 oracle's logits [STEPS][K][V], its greedy tokens) for one cell of the quality table."""
    from oracle.gen_golden import STATS_A, STATS_B
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    a = synth.make_args(preset)
    if weights == "default":
        sd = synth.make_state_dict(a, seed=0)
    else:
        sd = synth.trained_stats(synth.make_state_dict(a, seed=3, head_gain=4.0), a, **(STATS_A if weights == "trained_stats_A" else STATS_B))
    prompt = synth.random_prompt(a, 8, 20, seed=5)          # the length cap (10 frames per phoneme) ends the call after 60 steps
    tr = []
    VoiceCraftOracle(a, sd).inference_tts(*prompt, trace=tr, **KNOBS)
    want = torch.stack([t["logits"][0] for t in tr]).numpy()[:STEPS]
    toks = torch.stack([t["tokens"] for t in tr]).numpy()
    return a, sd, prompt, want, toks


def quality_figures(got, want):
    rel = rel_l2(got[1:], want[1:])                         # (step 0 reads no cache)
    agree = (got.argmax(-1) == want.argmax(-1)).all(axis=-1)
    return {"rel_l2_worst": round(float(rel.max()), 4), "rel_l2_median": round(float(np.median(rel)), 4),
            "teacher_forced_steps_agree": round(float(agree.mean()), 3)}


def quality_row(preset, weights):
    """{"kv8", "kv8c", "bf16"}: the three round trips of one cell against the plain oracle."""
    a, sd, prompt, want, toks = quality_setup(preset, weights)
    row = {"preset": preset, "weights": weights, "steps": int(len(want))}
    for tag in ("kv8", "kv8c", "bf16"):
        if tag == "kv8c":
            got = centred_tts_logits(Kv8cOracle(a, sd), prompt, toks)[:STEPS]
        else:
            got = kc.cached_tts_logits(kc.Kv8Oracle(a, sd, roundtrip=None if tag == "kv8" else (lambda t: t.bfloat16().float())), prompt, toks)[:STEPS]
        assert got.shape == want.shape and np.isfinite(got).all()
        row[tag] = quality_figures(got, want)
    return row


# ------------------------------------------------------------------------------------------------ the contract's scores, float64
def contract_scores(q, k_true, c, lo, scale):
    """Scores of one head's row as the contract assembles them: positions below lo from the 8-bit cache, (q . k8) 2^s + q . c, positions
    from lo up from the bf16 rows, uncentred; and the values each position stands for.  q [hd], k_true bf16-valued [S][hd], c [hd]."""
    from voicecraft_amd import quant
    kt = torch.as_tensor(k_true, dtype=torch.float32)
    ct = torch.as_tensor(c, dtype=torch.float32)
    codes, shift = quant.kv8c_quantize_rows(kt[:lo], ct)
    k8 = kc.grid_values(codes.numpy(), np.zeros_like(shift.numpy()))                       # the code bytes' own values, shift not applied
    q64 = np.asarray(q, dtype=np.float64) * scale
    s8 = (k8 @ q64) * 2.0 ** shift.numpy().astype(np.float64) + q64 @ ct.numpy().astype(np.float64)
    s16 = kt[lo:].numpy().astype(np.float64) @ q64
    stands_for = np.concatenate([ct.numpy().astype(np.float64)[None] + quant.kv8c_roundtrip(kt[:lo], ct).numpy().astype(np.float64),
                                 kt[lo:].numpy().astype(np.float64)])
    return np.concatenate([s8, s16]), stands_for


# ------------------------------------------------------------------------------------------------ kernel-level offsets
def launch_offsets(L, mult=20.0, seed=0):
    """c [n_seqs][H][hd], bf16-valued: about mult sigma per channel (sigma = the standard deviation of the launch's flat K numbers), signs
    and sizes of their own per head and sequence.  With a shared prefix every sequence takes sequence 0's."""
    rng = np.random.RandomState(991 + 13 * L.hd + seed)
    sigma = float(dc.content(L.hd, L.S_max + 1)[1].std())
    c = mult * sigma * rng.choice([-1.0, 1.0], size=(L.rows, dc.H, L.hd)) * rng.uniform(0.75, 1.25, size=(L.rows, dc.H, L.hd))
    if L.share:
        c[:] = c[0]
    return dc.bf16_exact(c)


BIG = 3.0e38
DEFECTS = ("missing", "doubled", "wrong_head", "wrong_seq")


def pass_entry(L, rps, c=None, defects=False):
    """A dc.Launch as a centred pass of `rps` rows per sequence, on the CPU: the arrays the kernel is handed, the float64
    reference and its bars, and the reference under each defect of q . c.

    The K a sequence holds is bf16(L.Kf + c): a common offset c [n_seqs][H][hd] per channel on every row.  The E4M3 array holds the codes
    of bf16_rne(k - c); the reference reads c + their values below lo and the bf16 rows from lo up.  Poison as in tests/test_gpu_kv8_attn.py:
    8-bit rows at positions >= lo hold the largest code at the largest shift, bf16 rows below lo hold 3e38, and what no row may read is
    NaN / the largest code.  A defect of q . c is a defect of the kernel, so it shows in every row of the launch at once: sens[defect] =
    the LARGEST over the rows (those that read both kinds of positions) of max_j |defective - ref|_j / bar_j, against the fp32-output and
    the bf16-output bar - what the launch's most telling row says (computed with defects=True only)."""
    from voicecraft_amd import quant
    assert L.family in ("flat", "probe", "peaked")
    hd, n_seq, S_max = L.hd, L.rows, L.S_max
    if c is None:
        c = launch_offsets(L)
    ct = torch.from_numpy(np.ascontiguousarray(c))
    K0, V = dc.kernel_caches(L)                                  # fp32, NaN where no row may read
    Kt = kc.bf16(torch.from_numpy(L.Kf[:, :, :S_max].copy()) + ct[:, :, None, :])      # every sequence's rows, offset
    Vt = torch.from_numpy(L.Vf[:, :, :S_max].copy())
    K = np.where(np.isnan(K0), np.nan, Kt.numpy())
    k8, ks = quant.kv8c_quantize_rows(Kt, ct)
    v8, vs = quant.kv8_quantize_rows(Vt)
    Kq = ct.numpy().astype(np.float64)[:, :, None, :] + quant.kv8c_roundtrip(Kt, ct).numpy().astype(np.float64)
    Vq = quant.kv8_dequantize(v8, vs).numpy()
    sh8 = torch.stack([ks, vs], dim=-1).contiguous()
    k8, v8 = k8.clone(), v8.clone()
    Kd, Vd = K.copy(), V.copy()
    row_seq, row_pos, q, ref, b32, b16, straddles = [], [], [], [], [], [], []
    sens = {d: [0.0, 0.0] for d in DEFECTS}
    scale = dc.kernel_scale(hd)
    for i in range(n_seq):
        s, last = int(L.row_seq[i]), int(L.row_pos[i])
        lo = last - rps + 1
        assert lo >= L.share and lo >= 0
        # peaked: does the sequence's run of equal maxima lie on both sides of lo (scored by two fp32 expressions once c != 0)?
        run = np.asarray(L.covered[i]) if L.family == "peaked" else None
        straddles += [bool(run is not None and run[0] < lo <= run[-1])] * rps
        for a8 in (k8, v8):
            a8[s, :, lo:] = 0x7e
            if s != 0:
                a8[s, :, :L.share] = 0x7e
        sh8[s, :, lo:] = 119
        if s != 0:
            sh8[s, :, :L.share] = 119
        for a in (Kd, Vd):
            a[s, :, (L.share if s else 0):lo] = BIG
        for j in range(rps):
            p = lo + j
            sh = min(L.share, p + 1) if s else 0
            Kr = np.concatenate([Kq[0, :, :sh], Kq[s, :, sh:lo], K[s, :, lo:p + 1]], axis=1).astype(np.float64)
            Vr = np.concatenate([Vq[0, :, :sh], Vq[s, :, sh:lo], V[s, :, lo:p + 1]], axis=1).astype(np.float64)
            assert Kr.shape[1] == p + 1 and np.isfinite(Kr).all() and np.isfinite(Vr).all()
            qr = L.q[(i + rps - 1 - j) % n_seq]
            qh = qr.reshape(dc.H, hd)
            ev = dc.row_eval(qh, Kr, Vr, hd)
            row_seq.append(s); row_pos.append(p); q.append(qr)
            ref.append(ev["out"].reshape(-1)); b32.append(dc.bars(ev, False).reshape(-1)); b16.append(dc.bars(ev, True).reshape(-1))
            if defects and lo > 0:                                # both kinds of positions: a wrong q . c moves the 8-bit scores alone
                qc = np.einsum("hd,shd->sh", qh.astype(np.float64), c.astype(np.float64)) * scale      # [seq][head]
                other = (s + 1) % n_seq
                deltas = {"missing": -qc[s], "doubled": qc[s], "wrong_head": qc[s][::-1] - qc[s]}
                if not L.share:
                    deltas["wrong_seq"] = qc[other] - qc[s]
                for name, dl in deltas.items():
                    sc = ev["sc"].copy()
                    sc[:, :lo] += dl[:, None]
                    e = np.exp(sc - sc.max(axis=1, keepdims=True))
                    out = np.einsum("hs,hsd->hd", e, Vr) / e.sum(axis=1)[:, None]
                    d = np.abs(out - ev["out"])
                    sens[name][0] = max(sens[name][0], float((d / dc.bars(ev, False)).max()))
                    sens[name][1] = max(sens[name][1], float((d / dc.bars(ev, True)).max()))
    if L.share:
        assert int(L.row_pos[list(L.row_seq).index(0)]) - rps + 1 >= L.share
    bf = torch.bfloat16
    return dict(name=f"{L.name}-rps{rps}", family=L.family, nsplit=L.nsplit, rps=rps, hd=hd, share=int(L.share),
                q=torch.from_numpy(np.stack(q)), K=torch.from_numpy(Kd).to(bf), V=torch.from_numpy(Vd).to(bf), k8=k8, v8=v8, sh8=sh8,
                centre=ct.to(bf).contiguous(), ref=np.stack(ref), b32=np.stack(b32), b16=np.stack(b16),
                seq_np=np.array(row_seq, dtype=np.int32), pos_np=np.array(row_pos, dtype=np.int32), sens=sens,
                straddles=np.array(straddles, dtype=bool))


def edge_entries(hd, families=("flat", "probe"), nsplits=dc.EDGE_NSPLITS, defects=False):
    out = []
    for n in nsplits:
        for rps in (1, 3):
            ls = kc.pass_lengths(hd, n, rps)
            for family in families:
                out.append(pass_entry(dc.make_launch("bf16", hd, n, family, ls), rps, defects=defects))
    return out


def share_entries(hd, defects=False):
    P, B = kc.PPW8[hd], kc.batch8(hd)
    out = []
    for n in dc.SHARE_NSPLITS:
        for rps in (1, 3):
            for sh in (1, P, B + 3):
                top = max(n * B + 7, sh + B + rps + 1)
                ls = sorted({sh + rps, sh + rps + 1, sh + P + rps, sh + B + rps + 1, top - 1})
                for family in ("flat", "probe"):
                    out.append(pass_entry(dc.make_launch("bf16", hd, n, family, ls + [top], share=sh, seed=1), rps, defects=defects))
    return out
