"""-m gpu: the kv8 form of rows_attn_k and the packer kv8_pack_k (voicecraft_amd/csrc/vc_attn.hip) through vc_debug_attn8, on the
generators, the float64 reference and the bars of tests/decode_attn_cases.py.

A PASS here is `rps` consecutive rows per sequence at consecutive positions; lo = the position of the sequence's first row.  The
reference is computed on the values each position must be read from: the quantiser's round trip of the bf16 rows below lo
(quant.kv8_quantize_rows, on the CPU), the bf16 rows from lo up.  The dequantised values are bf16 numbers, so the bars are the
module's own: 2^-18 max|V| for fp32 outputs, plus one bf16 rounding for bf16 outputs.
What must not be read is poisoned: the E4M3 rows and shifts at positions >= lo hold the largest code at the largest shift, the bf16
rows below lo hold 3e38, everything above a sequence's last position and - in sequences other than 0 - below the shared prefix is
NaN (bf16) or the largest code (E4M3): a wrong source is off by far more than a bar.
The peaked family rests on a run of EQUAL maxima at raw scores of +100: only because the run's scores are equal is the fp32 rounding of
a score of that size (2^-24 . 100 . a few, far more than 2^-18 as a weight error) common to them and gone from the normalised row.  A
run that straddles lo would hold quantised and unquantised copies of one K row, 3 % apart: its scores are no longer equal, and a plain
fp32 torch restatement of such a launch uses 0.73 of the bar by itself (0.15 once the rows are equal again).  So the peaked launches
get K rows that lie on the grid already (the quantiser's round trip, which is idempotent): both caches then hold the same numbers."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import decode_attn_cases as dc
import kv8_cases as kc

pytestmark = pytest.mark.gpu

SENT = 16384.0
DEV = "cuda:0"
BIG = 3.0e38
FORMS = [(nt, fast, p16) for nt in (0, 1) for fast in (1, 0) for p16 in (0, 1)]


def _i32(x):
    return torch.tensor(np.asarray(x, dtype=np.int32).reshape(-1), dtype=torch.int32, device=DEV)


def _pass_entry(L, rps):
    """A dc.Launch (row i = the LAST row of sequence row_seq[i], at position row_pos[i]) as a pass of rps rows per sequence."""
    from voicecraft_amd import quant
    if L.family == "peaked":
        L = dataclasses.replace(L, Kf=quant.kv8_roundtrip(torch.from_numpy(L.Kf.copy())).numpy())
    hd, n_seq, S_max = L.hd, L.rows, L.S_max
    K, V = dc.kernel_caches(L)                                   # fp32 [n_seqs][H][S_max][hd], NaN where no row may read
    Kt, Vt = torch.from_numpy(L.Kf[:, :, :S_max].copy()), torch.from_numpy(L.Vf[:, :, :S_max].copy())
    k8, ks = quant.kv8_quantize_rows(Kt)
    v8, vs = quant.kv8_quantize_rows(Vt)
    Kq, Vq = quant.kv8_dequantize(k8, ks).numpy(), quant.kv8_dequantize(v8, vs).numpy()
    sh8 = torch.stack([ks, vs], dim=-1).contiguous()
    k8, v8 = k8.clone(), v8.clone()
    Kd, Vd = K.copy(), V.copy()                                  # what the device's bf16 caches hold
    row_seq, row_pos, q, ref, b32, b16 = [], [], [], [], [], []
    for i in range(n_seq):
        s, last = int(L.row_seq[i]), int(L.row_pos[i])
        lo = last - rps + 1
        assert lo >= L.share and lo >= 0
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
            qr = L.q[(i + rps - 1 - j) % n_seq]                  # the sequence's last row keeps the q its lifted positions were built for
            ev = dc.row_eval(qr.reshape(dc.H, hd), Kr, Vr, hd)
            row_seq.append(s); row_pos.append(p); q.append(qr)
            ref.append(ev["out"].reshape(-1)); b32.append(dc.bars(ev, False).reshape(-1)); b16.append(dc.bars(ev, True).reshape(-1))
    if L.share:          # the prefix must be packed in sequence 0: its own first row lies behind it
        assert int(L.row_pos[list(L.row_seq).index(0)]) - rps + 1 >= L.share
    bf = torch.bfloat16
    return dict(name=f"{L.name}-rps{rps}", family=L.family, nsplit=L.nsplit, rps=rps, hd=hd, q=torch.from_numpy(np.stack(q)).to(DEV),
                K=torch.from_numpy(Kd).to(DEV).to(bf), V=torch.from_numpy(Vd).to(DEV).to(bf), k8=k8.to(DEV), v8=v8.to(DEV), sh8=sh8.to(DEV),
                row_seq=_i32(row_seq), row_pos=_i32(row_pos), share=_i32([L.share]), ref=np.stack(ref), b32=np.stack(b32),
                b16=np.stack(b16), seq_np=np.array(row_seq), pos_np=np.array(row_pos))


def _launch(e, nsplit, nt, fast, p16, x_out, n_active=1, row_seq=None, row_pos=None):
    from voicecraft_amd import engine
    return engine.debug_attn8(e["q"], e["K"], e["V"], e["k8"], e["v8"], e["sh8"], e["row_seq"] if row_seq is None else row_seq,
                              e["row_pos"] if row_pos is None else row_pos, _i32([n_active]), e["share"], nsplit, rps=e["rps"], nt=bool(nt),
                              fast=bool(fast), part16=bool(p16), x_out=x_out, sentinel=SENT)


def _rows(out):
    if "x_out" in out:
        x = out["x_out"].double().cpu().numpy()
        assert not (x == SENT).any(), "x_out elements left unwritten"
        return x
    o, ml = out["att_o"].double().cpu().numpy(), out["att_ml"].double().cpu().numpy()
    assert not (o == SENT).any() and not (ml == SENT).any(), "partials left unwritten"
    assert (ml[..., 1] >= 0).all() and not np.isnan(ml).any()
    assert (o[ml[..., 1] == 0] == 0).all(), "an empty split left a non-zero partial"
    return dc.merge(o, ml)


def _used(got, ref, bar, live=None):
    f = np.where(np.isfinite(got), np.abs(got - ref) / bar, np.inf)
    return float((f if live is None else f[live]).max())


def _judge(e, nt, fast, p16, worst):
    """Split partials (fp32, or bf16 with p16), and the unsplit bf16 x_out where nsplit == 1.  The flat family is held to fp32 outputs
    only, as in tests/test_gpu_decode_attn.py."""
    if not (p16 and e["family"] == "flat"):
        u = _used(_rows(_launch(e, e["nsplit"], nt, fast, p16, False)), e["ref"], e["b16"] if p16 else e["b32"])
        worst["partials"] = max(worst.get("partials", 0.0), u)
        assert u <= 1.0, (e["name"], "partials", dict(nt=nt, fast=fast, p16=p16), u)
    if e["nsplit"] == 1 and not p16 and e["family"] != "flat":
        u = _used(_rows(_launch(e, 1, nt, fast, 0, True)), e["ref"], e["b16"])
        worst["x_out"] = max(worst.get("x_out", 0.0), u)
        assert u <= 1.0, (e["name"], "x_out", dict(nt=nt, fast=fast), u)


@functools.lru_cache(maxsize=1)
def _edge_entries(hd):
    out = []
    for n in dc.EDGE_NSPLITS:
        for rps in (1, 3):
            ls = kc.pass_lengths(hd, n, rps)
            for family in ("flat", "probe", "peaked"):
                out.append(_pass_entry(dc.make_launch("bf16", hd, n, family, ls), rps))
    return out


@pytest.mark.parametrize("hd,nt,fast,p16", [(hd, *f) for hd in dc.HDS for f in FORMS])
def test_every_kv8_form_at_the_edges(hd, nt, fast, p16):
    """One compiled kv8 form at one head_dim: nsplit 1, 2, 3, 5, 7, 8; rps 1 and 3; context lengths around the positions per visit, the
    batch B8 = 4 * 8 * PPW8, n B8 and - at nsplit 8 - one past the first refill of the 8-way split; lengths whose last rps positions
    straddle a split edge."""
    worst = {}
    for e in _edge_entries(hd):
        _judge(e, nt, fast, p16, worst)
    print(f"\nkv8 hd {hd} nt {nt} fast {fast} p16 {p16}: fraction of the bar used {worst}")


@functools.lru_cache(maxsize=1)
def _share_entries(hd):
    P, B = kc.PPW8[hd], kc.batch8(hd)
    out = []
    for n in dc.SHARE_NSPLITS:
        for rps in (1, 3):
            for sh in (1, P, B + 3):
                top = max(n * B + 7, sh + B + rps + 1)
                ls = sorted({sh + rps, sh + rps + 1, sh + P + rps, sh + B + rps + 1, top - 1})
                for family in ("flat", "probe"):
                    out.append(_pass_entry(dc.make_launch("bf16", hd, n, family, ls + [top], share=sh, seed=1), rps))
    return out


@pytest.mark.parametrize("hd", dc.HDS)
def test_kv8_shared_prefix(hd):
    """share in {1, PPW8, B8 + 3} <= lo of every sequence: rows of sequence 0 and of others in one launch; the others hold poison below
    the prefix in both caches.  Every batch takes the general address path."""
    worst = {}
    for e in _share_entries(hd):
        assert int(e["share"]) > 0 and 0 in e["seq_np"] and (e["seq_np"] != 0).any()
        for nt, fast in ((0, 1), (1, 1), (0, 0)):
            for p16 in (0, 1):
                _judge(e, nt, fast, p16, worst)
    print(f"\nkv8 hd {hd} shared prefix: fraction of the bar used {worst}")


def test_kv8_rows_that_must_leave_nothing():
    """Whole sequences with pos = -1 (all rps rows), and *n_active = 0: empty partials, zero x_out rows; the live rows stay inside their bars."""
    hd = 64
    for n in (1, 3, 8):
        for rps in (1, 3):
            e = _pass_entry(dc.make_launch("bf16", hd, n, "probe", kc.pass_lengths(hd, n, rps)), rps)
            pos, seq = e["pos_np"].copy(), e["seq_np"].copy()
            n_seq = len(pos) // rps
            dead_seq = np.zeros(n_seq, dtype=bool)
            dead_seq[1::3] = True
            dead_seq[-1] = True
            dead = np.repeat(dead_seq, rps)
            pos[dead] = -1
            live = ~dead
            assert live.sum() >= 4 and dead.sum() >= 3
            for nt, fast, p16 in ((0, 1, 0), (1, 0, 0), (0, 1, 1)):
                for n_active in (1, 0):
                    alive = live if n_active else np.zeros_like(live)
                    out = _launch(e, n, nt, fast, p16, False, n_active=n_active, row_pos=_i32(pos))
                    o, ml = out["att_o"].double().cpu().numpy(), out["att_ml"].double().cpu().numpy()
                    assert (ml[~alive][..., 1] == 0).all() and (o[~alive] == 0).all(), (n, rps, nt, fast, p16, n_active)
                    if n_active:
                        assert _used(_rows(out), e["ref"], e["b16"] if p16 else e["b32"], live) <= 1.0
                    if n == 1 and not p16:
                        x = _rows(_launch(e, 1, nt, fast, 0, True, n_active=n_active, row_pos=_i32(pos)))
                        assert (x[~alive] == 0).all()
                        if n_active:
                            assert _used(x, e["ref"], e["b16"], live) <= 1.0


@pytest.mark.parametrize("hd", dc.HDS)
def test_pack_kernel_bit_equal_and_nothing_else_touched(hd):
    """kv8_pack_k: codes and shifts of the packed rows equal quant.kv8_quantize_rows bit for bit; every other byte of the three arrays keeps
    its preset; rows with pos = -1 and a launch with *n_active = 0 write nothing."""
    from voicecraft_amd import engine, quant
    n_seq, H, S_max = 5, 3, 70
    rows = torch.cat([kc.special_rows(hd), kc.random_rows(hd, 2 * n_seq * H * S_max, seed=3)])[: 2 * n_seq * H * S_max]
    rows = rows[torch.randperm(rows.shape[0], generator=torch.Generator().manual_seed(hd))]
    Kc, Vc = rows[: n_seq * H * S_max].reshape(n_seq, H, S_max, hd), rows[n_seq * H * S_max:].reshape(n_seq, H, S_max, hd)
    want = [quant.kv8_quantize_rows(t) for t in (Kc, Vc)]
    Kd, Vd = Kc.to(DEV).bfloat16().contiguous(), Vc.to(DEV).bfloat16().contiguous()
    rs = np.random.RandomState(hd)
    cells = [(s, p) for s in range(n_seq) for p in range(S_max)]
    pick = [cells[i] for i in rs.choice(len(cells), size=41, replace=False)]          # 41 rows: no multiple of the block's rows
    seq = np.array([c[0] for c in pick], dtype=np.int32)
    pos = np.array([c[1] for c in pick], dtype=np.int32)
    pos_in = pos.copy()
    pos_in[::7] = -1                                                                  # rows that carry nothing
    for n_active in (0, 1):
        k8 = torch.full((n_seq, H, S_max, hd), 0xA5, dtype=torch.uint8, device=DEV)
        v8 = torch.full_like(k8, 0x5A)
        sh = torch.full((n_seq, H, S_max, 2), 77, dtype=torch.int8, device=DEV)
        engine.debug_attn8(None, Kd, Vd, k8, v8, sh, _i32(seq), _i32(pos_in), _i32([n_active]), _i32([0]), pack=True)
        torch.cuda.synchronize()
        written = np.zeros((n_seq, S_max), dtype=bool)
        if n_active:
            written[seq[pos_in >= 0], pos_in[pos_in >= 0]] = True
        w = torch.from_numpy(written)[:, None, :].expand(n_seq, H, S_max)
        for got, preset, (wc, ws), j in ((k8.cpu(), 0xA5, want[0], 0), (v8.cpu(), 0x5A, want[1], 1)):
            assert torch.equal(got[w], wc[w]), (hd, n_active, j)
            assert bool((got[~w] == preset).all())
            s_got = sh.cpu()[..., j]
            assert torch.equal(s_got[w], ws[w]) and bool((s_got[~w] == 77).all())
        assert written.sum() == (int((pos_in >= 0).sum()) if n_active else 0)
