"""-m gpu: the centred forms of rows_attn_k and kv8_pack_k and the centre kernel kv8c_centre_k (voicecraft_amd/csrc/vc_attn.hip) through
vc_debug_attn8c, on the generators, the float64 reference and the bars of tests/decode_attn_cases.py / tests/kv8_cases.py
(tests/kv8c_cases.py pass_entry builds the passes on the CPU).

Every K row of a sequence carries a common offset of about 20 sigma per channel, another one per head and sequence; the E4M3 array holds
the codes of bf16_rne(k - c) and the reference reads c + their values below lo, the bf16 rows from lo up; everything else is poisoned
as in tests/test_gpu_kv8_attn.py.  What a missing, doubled, wrong-head or wrong-sequence q . c would do is shown on the CPU
(tests/test_kv8c_cpu.py test_a_wrong_qc_exceeds_the_bar): every launch here has a row that such a defect moves by at least 8 fp32 bars.

The peaked family's bar rests on a run of EQUAL scores of +100 whose fp32 rounding is common to the run (tests/test_gpu_kv8_attn.py).
Where the run straddles lo, one part of it is scored as q . k and the other as (q . k8) 2^s + q . c, two fp32 expressions that differ by
an ulp of 144 (log2 units): 8.6e-6 as a weight, more than the whole bar of 2^-18 = 3.8e-6, in ANY fp32 kernel once c != 0.  So the
peaked launches run with c != 0 on the sequences whose run lies wholly below lo or wholly from lo up (the others are given pos = -1, as
finished sequences are: both kinds must be there), and with c = 0 - where the two expressions are the same one and the centred form must
equal the kv8 form bit for bit - on all of them."""
import functools

import numpy as np
import pytest
import torch

import decode_attn_cases as dc
import kv8_cases as kc
import kv8c_cases as cc

pytestmark = pytest.mark.gpu

SENT = 16384.0
DEV = "cuda:0"
FORMS = [(nt, fast, p16) for nt in (0, 1) for fast in (1, 0) for p16 in (0, 1)]
TENSORS = ("q", "K", "V", "k8", "v8", "sh8", "centre")


def _i32(x):
    return torch.tensor(np.asarray(x, dtype=np.int32).reshape(-1), dtype=torch.int32, device=DEV)


def _dev(e):
    e = dict(e)
    for k in TENSORS:
        e[k] = e[k].to(DEV).contiguous()
    e["row_seq"], e["row_pos"], e["share_t"] = _i32(e["seq_np"]), _i32(e["pos_np"]), _i32([e["share"]])
    return e


def _launch(e, nsplit, nt, fast, p16, x_out, n_active=1, row_pos=None, centre=None):
    from voicecraft_amd import engine
    return engine.debug_attn8c(e["q"], e["K"], e["V"], e["k8"], e["v8"], e["sh8"], e["centre"] if centre is None else centre, e["row_seq"],
                               e["row_pos"] if row_pos is None else row_pos, _i32([n_active]), e["share_t"], nsplit, rps=e["rps"], mode=0,
                               nt=bool(nt), fast=bool(fast), part16=bool(p16), x_out=x_out, sentinel=SENT)


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
    """Split partials (fp32, or bf16 with p16), and the unsplit bf16 x_out where nsplit == 1; the flat family is held to fp32 outputs
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
    return [_dev(e) for e in cc.edge_entries(hd)]


@pytest.mark.parametrize("hd,nt,fast,p16", [(hd, *f) for hd in dc.HDS for f in FORMS])
def test_every_centred_form_at_the_edges(hd, nt, fast, p16):
    """One compiled centred form at one head_dim: nsplit 1, 2, 3, 5, 7, 8; rps 1 and 3; the context lengths of kv8_cases.pass_lengths."""
    worst = {}
    for e in _edge_entries(hd):
        _judge(e, nt, fast, p16, worst)
    print(f"\nkv8c hd {hd} nt {nt} fast {fast} p16 {p16}: fraction of the bar used {worst}")


@pytest.mark.parametrize("hd", dc.HDS)
def test_peaked_scores_under_a_centre(hd):
    """Raw scores between -120 and +100 with a non-zero q . c: the peaked launches of the edge table at nsplit 1, 3 and 8, every form.  A
    sequence whose run of maxima straddles lo is switched off (module docstring); runs wholly in the E4M3 cache and runs wholly in the
    pass's own bf16 rows both occur."""
    worst, below, above = 0.0, 0, 0
    for n in (1, 3, 8):
        for rps in (1, 3):
            L = dc.make_launch("bf16", hd, n, "peaked", kc.pass_lengths(hd, n, rps))
            e = _dev(cc.pass_entry(L, rps))
            live = ~e["straddles"]
            pos = e["pos_np"].copy()
            pos[~live] = -1
            for i in range(L.rows):
                if live[i * rps]:
                    lo = int(L.row_pos[i]) - rps + 1
                    below += int(L.covered[i][-1] < lo)
                    above += int(L.covered[i][0] >= lo)
            assert live.sum() >= 2 * rps, (n, rps)
            for nt, fast, p16 in FORMS:
                out = _launch(e, n, nt, fast, p16, False, row_pos=_i32(pos))
                o, ml = out["att_o"].double().cpu().numpy(), out["att_ml"].double().cpu().numpy()
                assert (ml[~live][..., 1] == 0).all() and (o[~live] == 0).all()
                u = _used(_rows(out), e["ref"], e["b16"] if p16 else e["b32"], live)
                worst = max(worst, u)
                assert u <= 1.0, (e["name"], dict(nt=nt, fast=fast, p16=p16), u)
                if n == 1 and not p16:
                    u = _used(_rows(_launch(e, 1, nt, fast, 0, True, row_pos=_i32(pos))), e["ref"], e["b16"], live)
                    assert u <= 1.0, (e["name"], "x_out", dict(nt=nt, fast=fast), u)
    assert below >= 10 and above >= 3, (below, above)
    assert float(e["centre"].float().abs().min()) > 0
    print(f"\nkv8c hd {hd} peaked, c != 0: fraction of the bar used {worst:.3f}; runs below lo {below}, from lo up {above}")


@functools.lru_cache(maxsize=1)
def _share_entries(hd):
    return [_dev(e) for e in cc.share_entries(hd)]


@pytest.mark.parametrize("hd", dc.HDS)
def test_centred_shared_prefix(hd):
    """share in {1, PPW8, B8 + 3}: rows of sequence 0 and of others in one launch, every sequence under sequence 0's centre; the others
    hold poison below the prefix in both caches."""
    worst = {}
    for e in _share_entries(hd):
        assert e["share"] > 0 and 0 in e["seq_np"] and (e["seq_np"] != 0).any()
        assert bool((e["centre"] == e["centre"][0]).all())
        for nt, fast in ((0, 1), (1, 1), (0, 0)):
            for p16 in (0, 1):
                _judge(e, nt, fast, p16, worst)
    print(f"\nkv8c hd {hd} shared prefix: fraction of the bar used {worst}")


def test_centred_rows_that_must_leave_nothing():
    """Whole sequences with pos = -1 (all rps rows), and *n_active = 0: empty partials, zero x_out rows; the live rows stay inside their bars."""
    hd = 64
    for n in (1, 3, 8):
        for rps in (1, 3):
            e = _dev(cc.pass_entry(dc.make_launch("bf16", hd, n, "probe", kc.pass_lengths(hd, n, rps)), rps))
            pos = e["pos_np"].copy()
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
def test_a_zero_centre_is_the_kv8_form(hd):
    """c = 0 (this test is blind to q . c and is here for equality only): on the arrays of tests/test_gpu_kv8_attn.py's passes - the peaked
    family among them - every centred form returns what the kv8 form returns, bit for bit."""
    from voicecraft_amd import engine
    import test_gpu_kv8_attn as t8
    for n in (1, 3, 8):
        for rps in (1, 3):
            for family in ("probe", "peaked"):
                e = t8._pass_entry(dc.make_launch("bf16", hd, n, family, kc.pass_lengths(hd, n, rps)), rps)
                zero = torch.zeros((e["K"].shape[0], dc.H, hd), dtype=torch.bfloat16, device=DEV)
                for nt, fast, p16 in FORMS:
                    for x_out in ((False, True) if n == 1 and not p16 else (False,)):
                        nn = 1 if x_out else n
                        args = (e["row_seq"], e["row_pos"], _i32([1]), e["share"], nn)
                        kw = dict(rps=rps, nt=bool(nt), fast=bool(fast), part16=bool(p16), x_out=x_out, sentinel=SENT)
                        a = engine.debug_attn8(e["q"], e["K"], e["V"], e["k8"], e["v8"], e["sh8"], *args, **kw)
                        b = engine.debug_attn8c(e["q"], e["K"], e["V"], e["k8"], e["v8"], e["sh8"], zero, *args, mode=0, **kw)
                        for k in a:
                            assert torch.equal(a[k].view(torch.int16 if a[k].dtype == torch.bfloat16 else torch.int32),
                                               b[k].view(torch.int16 if b[k].dtype == torch.bfloat16 else torch.int32)), (family, n, rps, nt, fast, p16, k)


@pytest.mark.parametrize("hd", dc.HDS)
def test_centred_packer_bit_equal_and_nothing_else_touched(hd):
    """kv8_pack_k<centred>: K codes and shifts of the packed rows equal quant.kv8c_quantize_rows, V codes and shifts quant.kv8_quantize_rows,
    bit for bit; every other byte of the three arrays keeps its preset; rows with pos = -1 and a launch with *n_active = 0 write nothing."""
    from voicecraft_amd import engine, quant
    n_seq, H, S_max = 5, 3, 70
    rows = torch.cat([kc.special_rows(hd), kc.random_rows(hd, 2 * n_seq * H * S_max, seed=3)])[: 2 * n_seq * H * S_max]
    rows = rows[torch.randperm(rows.shape[0], generator=torch.Generator().manual_seed(hd))]
    base, Vc = rows[: n_seq * H * S_max].reshape(n_seq, H, S_max, hd), rows[n_seq * H * S_max:].reshape(n_seq, H, S_max, hd)
    g = torch.Generator().manual_seed(5 + hd)
    sig = base.abs().median()
    c = kc.bf16(20.0 * sig * torch.where(torch.rand(n_seq, H, hd, generator=g) < 0.5, -1.0, 1.0) * (0.75 + 0.5 * torch.rand(n_seq, H, hd, generator=g)))
    c[1] = 0.0                                                                        # one sequence with the centre of nothing
    Kc = kc.bf16(base + c[:, :, None, :]).clamp(-3.0e38, 3.0e38)
    Kc[1] = base[1]
    want = [quant.kv8c_quantize_rows(Kc, c), quant.kv8_quantize_rows(Vc)]
    assert not torch.equal(want[0][0], quant.kv8_quantize_rows(Kc)[0])
    Kd, Vd, cd = Kc.to(DEV).bfloat16().contiguous(), Vc.to(DEV).bfloat16().contiguous(), c.to(DEV).bfloat16().contiguous()
    rs = np.random.RandomState(hd)
    cells = [(s, p) for s in range(n_seq) for p in range(S_max)]
    pick = [cells[i] for i in rs.choice(len(cells), size=41, replace=False)]          # 41 rows: no multiple of the block's rows
    seq = np.array([x[0] for x in pick], dtype=np.int32)
    pos = np.array([x[1] for x in pick], dtype=np.int32)
    pos_in = pos.copy()
    pos_in[::7] = -1                                                                  # rows that carry nothing
    for n_active in (0, 1):
        k8 = torch.full((n_seq, H, S_max, hd), 0xA5, dtype=torch.uint8, device=DEV)
        v8 = torch.full_like(k8, 0x5A)
        sh = torch.full((n_seq, H, S_max, 2), 77, dtype=torch.int8, device=DEV)
        engine.debug_attn8c(None, Kd, Vd, k8, v8, sh, cd, _i32(seq), _i32(pos_in), _i32([n_active]), _i32([0]), mode=1)
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
        assert torch.equal(cd.cpu(), c.bfloat16()), "the packer reads the centres"


N0S = (1, 2, 63, 64, 65, 2048)          # 2048 = VC_MAX_ROWS, the largest prefill pass the engine issues


@pytest.mark.parametrize("hd", dc.HDS)
def test_centre_kernel(hd):
    """kv8c_centre_k over a pass as prefill_batch lays it out (prompts back to back, each on a multiple of 16 rows, padding rows at
    pos = -1): sequences that start at 0 with n0 = 1, 2, 63, 64, 65 rows and - in a pass of its own - 2048; a sequence that enters the pass
    at position 7 (the later pass of a long prompt), which must keep its centre; a slot without rows.  Bar: |c - mean64| <= 2^-8 |mean64| +
    2^-20 max|k| - one bf16 rounding plus fp32 summation.  n0 comes back per slot.  *n_active == 0: nothing is written.  While
    *share_len > 0 every slot with a row in the pass takes sequence 0's centre and n0, in the pass that holds sequence 0's position 0
    and in a later one."""
    from voicecraft_amd import engine
    H = 2
    g = torch.Generator().manual_seed(hd)
    PRESET, ROWS0 = 7.0, -5

    def run(lengths, starts, n_slots, share=0, n_active=1, centre=None, n0=None, S_max=None):
        """lengths / starts per slot in pass order (length 0: the slot has no row)."""
        S_max = S_max or max(st + ln for st, ln in zip(starts, lengths)) + 3
        K = kc.bf16(torch.randn(n_slots, H, S_max, hd, generator=g) * 0.5 + 4.0 * torch.randn(n_slots, H, 1, hd, generator=g))
        seq, pos = [], []
        for s, (st, ln) in enumerate(zip(starts, lengths)):
            seq += [s] * ln + [0] * (-ln % 16)
            pos += list(range(st, st + ln)) + [-1] * (-ln % 16)
        if centre is None:
            centre = torch.full((n_slots, H, hd), PRESET, dtype=torch.bfloat16, device=DEV)
            n0 = torch.full((n_slots,), ROWS0, dtype=torch.int32, device=DEV)
        engine.debug_attn8c(None, K.to(DEV).bfloat16().contiguous(), None, None, None, None, centre, _i32(seq), _i32(pos), _i32([n_active]),
                            _i32([share]), mode=2, n0=n0)
        torch.cuda.synchronize()
        return K, centre, n0

    def held(c, K, s, ln):
        m = K[s, :, :ln].double().mean(dim=1)
        bar = 2.0 ** -8 * m.abs() + 2.0 ** -20 * K[s, :, :ln].abs().max()
        err = (c.double() - m).abs()
        assert bool((err <= bar).all()), (hd, s, ln, float((err / bar).max()))
        return float((err / bar).max())

    worst = 0.0
    # slots 0..4 start at 0; slot 5 enters at position 7; slot 6 has no row; slot 7 starts at 0 again
    lengths, starts = [1, 2, 63, 64, 65, 30, 0, 17], [0, 0, 0, 0, 0, 7, 0, 0]
    K, c, n0 = run(lengths, starts, 8)
    c, n0 = c.float().cpu(), n0.cpu()
    for s, ln in enumerate(lengths):
        if starts[s] == 0 and ln:
            worst = max(worst, held(c[s], K, s, ln))
            assert int(n0[s]) == ln
        else:
            assert bool((c[s] == PRESET).all()) and int(n0[s]) == ROWS0, ("left untouched", s)
    K, c, n0 = run(lengths, starts, 8, n_active=0)
    assert bool((c.float().cpu() == PRESET).all()) and bool((n0.cpu() == ROWS0).all()), "*n_active == 0 writes nothing"
    # the largest pass: one sequence of 2048 rows
    K, c, n0 = run([2048], [0], 2)
    worst = max(worst, held(c.float().cpu()[0], K, 0, 2048))
    assert int(n0[0]) == 2048 and bool((c.float().cpu()[1] == PRESET).all()) and int(n0[1]) == ROWS0
    # a shared prefix: slots 0, 1, 3 in the pass (1 and 3 behind the prefix), slot 2 absent -> 0, 1, 3 hold slot 0's centre
    K, c, n0 = run([40, 9, 0, 21], [0, 12, 0, 12], 4, share=12)
    cc_, nn = c.float().cpu(), n0.cpu()
    worst = max(worst, held(cc_[0], K, 0, 40))
    assert torch.equal(cc_[1], cc_[0]) and torch.equal(cc_[3], cc_[0]) and nn.tolist() == [40, 40, ROWS0, 40]
    assert bool((cc_[2] == PRESET).all())
    # ... and a later pass of the same call without sequence 0: slot 2 takes what slot 0 holds, slot 0 keeps it
    before = c.clone()
    K2, c, n0 = run([0, 0, 25, 0], [0, 0, 12, 0], 4, share=12, centre=c, n0=n0, S_max=K.shape[2])
    assert torch.equal(c[2], before[0]) and torch.equal(c[[0, 1, 3]], before[[0, 1, 3]]) and n0.cpu().tolist() == [40, 40, 40, 40]
    print(f"\nkv8c centre kernel hd {hd}: fraction of the bar used {worst:.3f}")
