"""rows_attn_k against float64, position by position (tests/decode_attn_cases.py holds the cases, the reference, the bars and the
proof that a kernel inside its bar has not lost, doubled or misplaced a covered position; tests/test_decode_attn_cpu.py runs it).

The kernel is launched through vc_debug_attn on buffers of the test: H = 2 heads, many rows per launch, each row at its own context
length in its own sequence slot (seq != row).  Every position a row must not read is NaN.  Split forms are merged on the host in
float64; only the merged row is judged, per element, against
    fp32 outputs   2^-18 max|V|                              bf16 outputs   that + 2^-8 sum_p w_p |V_pj|
Each test prints the largest fraction of the bar the kernel used next to the fraction a plain fp32 torch restatement of the same
rows uses."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import decode_attn_cases as dc

pytestmark = pytest.mark.gpu

SENT = 16384.0          # preset of every output buffer (exact in bf16): an unwritten partial shows
DEV = "cuda:0"
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
FORMS = [(dtype, nt, fast, p16) for dtype in dc.DTYPES for nt in (0, 1) for fast in (1, 0) for p16 in ((0, 1) if dtype == "bf16" else (0,))]
assert len(FORMS) == 12          # the compiled forms of rows_attn_k


def _i32(x):
    return torch.tensor(np.asarray(x, dtype=np.int32).reshape(-1), dtype=torch.int32, device=DEV)


def _launch(e, nsplit, nt, fast, p16, x_out, n_active=1, row_seq=None, row_pos=None):
    from voicecraft_amd import engine
    return engine.debug_attn(e["q"], e["K"], e["V"], e["row_seq"] if row_seq is None else row_seq,
                             e["row_pos"] if row_pos is None else row_pos, _i32([n_active]), e["share"], nsplit, nt=bool(nt),
                             fast=bool(fast), part16=bool(p16), x_out=x_out, sentinel=SENT)


def _rows(out):
    """The launch's rows in float64 [rows][H * hd]: x_out as it is, partials merged on the host; nothing may be left unwritten."""
    if "x_out" in out:
        x = out["x_out"].double().cpu().numpy()
        assert not (x == SENT).any(), "x_out elements left unwritten"
        return x
    o, ml = out["att_o"].double().cpu().numpy(), out["att_ml"].double().cpu().numpy()
    assert not (o == SENT).any() and not (ml == SENT).any(), "partials left unwritten"
    assert (ml[..., 1] >= 0).all() and not np.isnan(ml).any()
    dead = ml[..., 1] == 0
    assert (o[dead] == 0).all(), "an empty split left a non-zero partial"
    return dc.merge(o, ml)


def _used(got, ref, bar, live=None):
    """Largest |got - ref| / bar over the (live) rows; a NaN or an infinity counts as infinitely far."""
    f = np.abs(got - ref) / bar
    f = np.where(np.isfinite(got), f, np.inf)
    return float((f if live is None else f[live]).max())


def _device_entry(L):
    K, V = dc.kernel_caches(L)
    ref, b32, b16 = dc.reference(L, K, V)
    t = TDT[L.dtype]
    return dict(name=L.name, family=L.family, nsplit=L.nsplit, rows=L.rows, hd=L.hd, dtype=L.dtype,
                q=torch.from_numpy(L.q).to(DEV), K=torch.from_numpy(K).to(DEV).to(t), V=torch.from_numpy(V).to(DEV).to(t),
                row_seq=_i32(L.row_seq), row_pos=_i32(L.row_pos), share=_i32([L.share]), ref=ref, b32=b32, b16=b16,
                seq_np=L.row_seq.copy(), restated=_used(dc.restate_fp32(L, K, V), ref, b32))


def _judge(e, nt, fast, p16, worst):
    """One entry in one kernel form: split partials, and the unsplit x_out where nsplit == 1.  The flat family is held to fp32 outputs
    only (it does not separate one position from a bf16 rounding)."""
    bf16_x = e["dtype"] == "bf16"
    if not (p16 and e["family"] == "flat"):
        u = _used(_rows(_launch(e, e["nsplit"], nt, fast, p16, False)), e["ref"], e["b16"] if p16 else e["b32"])
        worst["partials"] = max(worst.get("partials", 0.0), u)
        assert u <= 1.0, (e["name"], "partials", dict(nt=nt, fast=fast, p16=p16), u)
    if e["nsplit"] == 1 and not p16 and not (bf16_x and e["family"] == "flat"):
        u = _used(_rows(_launch(e, 1, nt, fast, 0, True)), e["ref"], e["b16"] if bf16_x else e["b32"])
        worst["x_out"] = max(worst.get("x_out", 0.0), u)
        assert u <= 1.0, (e["name"], "x_out", dict(nt=nt, fast=fast), u)


# ------------------------------------------------------------------------------------------------ every length
@pytest.mark.parametrize("hd", dc.HDS)
@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_every_context_length(dtype, hd):
    """Flat family, EVERY S = 1 .. 8 * 4 * 8 * PPW + 65 (one past the first refill of an 8-way split), nsplit 1..8, default form
    (fast, no non-temporal hint), fp32 partials; fp32 caches also the unsplit x_out.  64 context lengths per launch."""
    from voicecraft_amd import engine
    top = dc.sweep_top(dtype, hd)
    cq, cK, cV = dc.content(hd, top + 1)
    ref, bar = dc.sweep_reference(dtype, hd)
    t = TDT[dtype]
    base_k = torch.from_numpy(cK[:, :, :top].copy()).to(DEV).to(t)
    base_v = torch.from_numpy(cV[:, :, :top].copy()).to(DEV).to(t)
    R = 64
    kc, vc = torch.empty((R, dc.H, top, hd), dtype=t, device=DEV), torch.empty((R, dc.H, top, hd), dtype=t, device=DEV)
    p_idx = torch.arange(top, device=DEV).view(1, 1, top, 1)
    row_seq = np.array([(i + 1) % R for i in range(R)], dtype=np.int32)
    one, zero = _i32([1]), _i32([0])
    got = {}          # (n or "x") -> list of (lengths, rows)
    for lo in list(range(1, top - R + 1, R)) + [top - R + 1]:
        lengths = np.arange(lo, lo + R)
        fill = np.empty(R, dtype=np.int64)
        fill[row_seq] = lengths                                       # sequence s holds positions 0 .. fill[s] - 1
        beyond = p_idx >= torch.from_numpy(fill).to(DEV).view(R, 1, 1, 1)
        for c, b in ((kc, base_k), (vc, base_v)):
            c[0], c[1:] = b[0], b[1]
            c.masked_fill_(beyond, float("nan"))
        q = torch.from_numpy(np.stack([cq[(S - 1) % dc.NQ].reshape(-1) for S in lengths])).to(DEV)
        args = (q, kc, vc, _i32(row_seq), _i32(lengths - 1), one, zero)
        for n in range(1, dc.MAX_NSPLIT + 1):
            got.setdefault(n, []).append((lengths, _rows(engine.debug_attn(*args, n, sentinel=SENT))))
        if dtype == "fp32":
            got.setdefault("x", []).append((lengths, _rows(engine.debug_attn(*args, 1, x_out=True, sentinel=SENT))))
    seen = np.zeros(top + 1, dtype=bool)
    worst = {}
    for key, parts in got.items():
        for lengths, rows in parts:
            seen[lengths] = True
            c = np.where(row_seq == 0, 0, 1)
            want = ref[c, (lengths - 1) % dc.NQ, lengths - 1]
            b = np.repeat(bar[c, lengths - 1], hd, axis=1)
            f = np.where(np.isfinite(rows), np.abs(rows - want) / b, np.inf).max(axis=1)
            i = int(f.argmax())
            if f[i] > worst.get(key, (0.0, 0))[0]:
                worst[key] = (float(f[i]), int(lengths[i]))
    assert seen[1:].all()
    L = dc.sweep_launch(dtype, hd, [top - 1, top])
    r, b32, _ = dc.reference(L)
    print(f"\n{dtype} hd {hd}, S = 1..{top}: fraction of the fp32 bar used, (worst, at S) per nsplit / x_out: {worst}; "
          f"fp32 restatement at the longest rows: {_used(dc.restate_fp32(L), r, b32):.3f}")
    assert max(v[0] for v in worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------ every compiled form at the edges
@functools.lru_cache(maxsize=1)
def _edge_entries(dtype, hd):
    return [_device_entry(L) for n in dc.EDGE_NSPLITS for L in dc.edge_launches(dtype, hd, n).values()]


@pytest.mark.parametrize("hd,dtype,nt,fast,p16", [(hd, *f) for dtype in dc.DTYPES for hd in dc.HDS for f in FORMS if f[0] == dtype])
def test_every_form_at_the_edges(hd, dtype, nt, fast, p16):
    """One compiled form of rows_attn_k at one head_dim: nsplit 1, 2, 3, 5, 7, 8; S = 1, 2, n - 1, n, n + 1, PPW +- 1, 8 PPW +- 1, B - 1,
    B, B + 1, n B - 1, n B, n B + 1, 2 B + 1 (B = 4 * 8 * PPW), an S whose last split is empty, S_max; flat (fp32 outputs), probe and peaked."""
    worst, restated = {}, {}
    for e in _edge_entries(dtype, hd):
        _judge(e, nt, fast, p16, worst)
        restated[e["family"]] = round(max(restated.get(e["family"], 0.0), e["restated"]), 3)
    print(f"\n{dtype} hd {hd} nt {nt} fast {fast} p16 {p16}: fraction of the bar used {worst}; fp32 restatement (fp32 bar) {restated}")


# ------------------------------------------------------------------------------------------------ shared prefix
@functools.lru_cache(maxsize=1)
def _share_entries(dtype, hd):
    return [_device_entry(dc.share_launch(dtype, hd, n, share, family)) for n in dc.SHARE_NSPLITS for share in dc.share_values(dtype, hd)
            for family in ("flat", "probe")]


@pytest.mark.parametrize("hd", dc.HDS)
@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_shared_prefix(dtype, hd):
    """share in {1, PPW, B + 3, pos}: rows of sequence 0 and of other sequences in one launch, contexts shorter than the prefix, ending at
    it, just behind it and a refill behind it; nsplit 1, 4, 8.  Every batch takes the general address path here (the lean first batch
    is what every other test of this file runs).  The other sequences hold NaN below the prefix."""
    worst, restated = {}, {}
    for e in _share_entries(dtype, hd):
        assert int(e["share"]) > 0 and 0 in e["seq_np"] and (e["seq_np"] != 0).any()
        for nt, fast in ((0, 1), (1, 1), (0, 0)):
            for p16 in ((0, 1) if dtype == "bf16" else (0,)):
                _judge(e, nt, fast, p16, worst)
        restated[e["family"]] = round(max(restated.get(e["family"], 0.0), e["restated"]), 3)
    print(f"\n{dtype} hd {hd} shared prefix: fraction of the bar used {worst}; fp32 restatement (fp32 bar) {restated}")


# ------------------------------------------------------------------------------------------------ rows that must leave nothing
@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_rows_that_must_leave_nothing(dtype):
    """pos = -1 and seq = -1 rows mixed with live ones, and a whole launch with *n_active = 0: their partials are (L, O) = (0, 0), their
    x_out rows 0; the live rows stay inside their bars."""
    hd = 64
    for n in (1, 3, 8):
        L = dc.make_launch(dtype, hd, n, "probe", dc.edge_lengths(dtype, hd, n))
        e = _device_entry(L)
        pos, seq = L.row_pos.copy(), L.row_seq.copy()
        pos[1::4] = -1
        seq[3::4] = -1
        pos[-1], seq[0] = -1, -1          # the longest row and the first one
        live = (pos >= 0) & (seq >= 0)
        assert live.sum() >= 4 and (~live).sum() >= 4
        for nt, fast, p16 in ((0, 1, 0), (1, 0, 0)) + (((0, 1, 1),) if dtype == "bf16" else ()):
            for n_active in (1, 0):
                alive = live if n_active else np.zeros_like(live)
                out = _launch(e, n, nt, fast, p16, False, n_active=n_active, row_seq=_i32(seq), row_pos=_i32(pos))
                o, ml = out["att_o"].double().cpu().numpy(), out["att_ml"].double().cpu().numpy()
                assert (ml[~alive][..., 1] == 0).all() and (o[~alive] == 0).all(), (n, nt, fast, p16, n_active)
                if n_active:
                    assert _used(_rows(out), e["ref"], e["b16"] if p16 else e["b32"], live) <= 1.0
                if n == 1 and not p16:
                    x = _rows(_launch(e, 1, nt, fast, 0, True, n_active=n_active, row_seq=_i32(seq), row_pos=_i32(pos)))
                    assert (x[~alive] == 0).all()
                    if n_active:
                        assert _used(x, e["ref"], e["b16"] if dtype == "bf16" else e["b32"], live) <= 1.0


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_with_real_buffers():
    """What no decode pass can issue is refused (VC_EINVAL) before anything is launched: the output buffers keep their preset."""
    from voicecraft_amd import _lib
    lib = _lib.load()
    hd, S_max, rows, n = 64, 128, 3, 4
    q = torch.zeros((rows, dc.H * hd), device=DEV)
    kc = torch.zeros((rows, dc.H, S_max, hd), dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    att_o, att_ml = torch.full((rows, dc.H, n, hd), SENT, device=DEV), torch.full((rows, dc.H, n, 2), SENT, device=DEV)
    x = torch.full((rows, dc.H * hd), SENT, dtype=torch.bfloat16, device=DEV)
    seq, pos, one, zero = _i32([1, 2, 0]), _i32([5, 0, 100]), _i32([1]), _i32([0])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        base = dict(q=q.data_ptr(), kcache=kc.data_ptr(), vcache=vc.data_ptr(), row_seq=seq.data_ptr(), row_pos=pos.data_ptr(),
                    n_active=one.data_ptr(), share_len=zero.data_ptr(), att_o=att_o.data_ptr(), att_ml=att_ml.data_ptr(), x_out=None,
                    dtype=1, H=dc.H, hd=hd, S_max=S_max, rows=rows, nsplit=n, nt=0, fast=1, part16=0)
        base.update(kw)
        return lib.vc_debug_attn(C.byref(_lib.DebugAttnArgs(**base)), stream)

    for kw in (dict(hd=48), dict(hd=16), dict(hd=256), dict(nsplit=0), dict(nsplit=9), dict(x_out=x.data_ptr()),
               dict(x_out=x.data_ptr(), nsplit=1, part16=1), dict(part16=1, dtype=0), dict(q=None), dict(kcache=None), dict(vcache=None),
               dict(row_seq=None), dict(row_pos=None), dict(n_active=None), dict(share_len=None), dict(att_o=None), dict(att_ml=None)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (att_o == SENT).all() and (att_ml == SENT).all() and (x == SENT).all()
    assert call() == 0 and call(part16=1) == 0 and call(x_out=x.data_ptr(), nsplit=1) == 0          # and the legal neighbours run
    torch.cuda.synchronize()
    assert not (att_ml == SENT).any() and not (x == SENT).any()
