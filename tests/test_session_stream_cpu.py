"""CPU: the streaming boundary of decode sessions and of the codec without a GPU (include/vc_engine.h vc_session_frames,
include/vc_codec.h vc_codec_decode_streams*): the symbols are exported and bound and refuse bad arguments without touching a device,
the new kernels are in the compiled gfx950 code without scratch, and SessionStreamer's id free list holds against a stub session."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_store_scan as isa  # noqa: E402

CODEC_SYMBOLS = ("vc_codec_decode_streams_open", "vc_codec_decode_streams_reset", "vc_codec_decode_streams", "vc_codec_last_streams_census")


@pytest.fixture(scope="module")
def lib():
    from voicecraft_amd import _lib, codec
    return codec._bind(_lib.load())


def test_symbols_are_exported_bound_and_refuse_bad_arguments(lib):
    from voicecraft_amd import _lib, codec
    assert hasattr(lib, "vc_session_frames") and _lib.PROTOTYPES["vc_session_frames"][0] is C.c_int
    assert len(_lib.PROTOTYPES["vc_session_frames"][1]) == 9
    for name in CODEC_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in codec.PROTOTYPES and codec.PROTOTYPES[name][0] is C.c_int, name
    t, a, b, d = (C.c_int * 1)(1), (C.c_int * 1)(), (C.c_int * 1)(), (C.c_int * 1)()
    assert lib.vc_session_frames(None, 1, t, 1, None, 8, a, b, d) == -1
    assert lib.vc_session_frames(None, 0, None, 0, None, 0, None, None, None) == -1
    assert lib.vc_codec_decode_streams_open(None, 1) == -1
    assert lib.vc_codec_decode_streams_reset(None, 0) == -1
    assert lib.vc_codec_decode_streams(None, 1, t, None, a, b, d, None, a, b, None) == -1
    assert lib.vc_codec_last_streams_census(None, (C.c_int * 4)()) == -1
    # a handle that was never finalized: refused before any device work
    h = C.c_void_p()
    rc = lib.vc_codec_create(C.byref(codec.make_cfg()), 0, C.byref(h))
    if rc == 0:                      # (a device is present: the handle exists, unfinalized)
        assert lib.vc_codec_decode_streams_open(h, 1) == -2
        assert lib.vc_codec_decode_streams_reset(h, 0) == -2
        assert lib.vc_codec_decode_streams(h, 1, t, None, a, b, d, None, a, b, None) == -2
        assert lib.vc_codec_last_streams_census(h, None) == -1
        lib.vc_codec_destroy(h)


def test_python_surface_is_importable():
    import voicecraft_amd
    from voicecraft_amd import DecodeSession, SessionStreamer
    from voicecraft_amd.codec import AudioTokenizer, CodecDecodeStreams
    import inspect
    assert callable(DecodeSession.poll_frames) and "stream" in inspect.signature(DecodeSession.submit).parameters
    assert "stream" not in inspect.signature(DecodeSession.submit_edit).parameters          # editing requests do not stream
    assert callable(AudioTokenizer.decode_streams)
    for m in ("feed", "reset", "ready_frames", "census"):
        assert callable(getattr(CodecDecodeStreams, m)), m
    assert voicecraft_amd.SessionStreamer is SessionStreamer and callable(SessionStreamer.pump)


def _kernels(unit, tmp_path):
    src = os.path.join(ROOT, "voicecraft_amd", "csrc", unit + ".hip")
    dst = str(tmp_path / (unit + ".s"))
    r = subprocess.run([isa.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S", src, "-o", dst],
                       cwd=os.path.dirname(src), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return {isa.demangle(n).replace("void ", ""): v for n, v in isa.kernels(open(dst).read()).items()}


@pytest.mark.skipif(not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)), reason="hipcc not available")
@pytest.mark.parametrize("unit,names", [("vc_tokens", ("session_gather_k(",)),
                                        ("vc_codec", ("streams_window_k(", "streams_state_k(", "streams_keep_emit_k("))])
def test_the_new_kernels_are_compiled_for_gfx950_without_scratch(unit, names, tmp_path):
    kern = _kernels(unit, tmp_path)
    for prefix in names:
        sel = {n: v for n, v in kern.items() if n.startswith(prefix)}
        assert len(sel) == 1, (prefix, sorted(kern))
        for name, (body, scratch, vgpr) in sel.items():
            assert scratch == 0 and "scratch_" not in body, (name, scratch)


# ------------------------------------------------------------------------------------------------ SessionStreamer's id free list
class _StubStreams:
    def __init__(self, n):
        self.n, self.active, self.resets, self.feeds, self.max_active = n, set(), [], 0, 0
        self.dirty = set()

    def reset(self, sid):
        assert sid not in self.active
        self.resets.append(sid)
        self.dirty.discard(sid)

    def feed(self, chunks, last=()):
        self.feeds += 1
        for sid in set(chunks) | set(last):
            assert 0 <= sid < self.n
            assert sid in self.active or sid not in self.dirty, f"stream {sid} reused without a reset"
            self.active.add(sid)
            self.dirty.add(sid)
        self.max_active = max(self.max_active, len(self.active))
        out = {sid: torch.zeros((1, 1, 3 * (chunks[sid].shape[2] if sid in chunks else 0))) for sid in set(chunks) | set(last)}
        for sid in last:
            self.active.discard(sid)
        return out


class _StubTok:
    device = torch.device("cpu")
    n_q = 4

    def __init__(self):
        self.streams = None

    def decode_streams(self, n):
        self.streams = _StubStreams(n)
        return self.streams


class _StubSession:
    """max_live slots; ticket t produces length[t] frames, 2 per turn once admitted (FIFO), is reported finished by the turn after
    its last frame and hands its last frames out with done = True."""

    def __init__(self, max_live, lengths):
        self.max_live, self.lengths = max_live, dict(lengths)
        self.pending, self.live, self.made, self.given = sorted(lengths), [], {}, {}
        self.idle = False

    def poll(self):
        out = []
        for t in list(self.live):
            if self.made[t] >= self.lengths[t] and self.given[t] >= self.lengths[t]:
                self.live.remove(t)
                out.append((t, None, None))
        while self.pending and len(self.live) < self.max_live:
            t = self.pending.pop(0)
            self.live.append(t)
            self.made[t] = self.given[t] = 0
        for t in self.live:
            self.made[t] = min(self.lengths[t], self.made[t] + 2)
        self.idle = not self.live and not self.pending
        return out

    def poll_frames(self, chunk):
        out = []
        for t in self.live:
            n = self.made[t] - self.given[t]
            ended = self.made[t] >= self.lengths[t]
            if n >= chunk or (ended and self.given[t] < self.lengths[t]):
                out.append((t, self.given[t], torch.zeros((1, 4, n), dtype=torch.int64), ended))
                self.given[t] += n
        return out


def test_session_streamer_reuses_an_id_only_after_done_and_never_holds_more_than_max_live():
    from voicecraft_amd.stream import SessionStreamer
    lengths = {t: 3 + (5 * t) % 11 for t in range(1, 15)}
    sess, tok = _StubSession(3, lengths), _StubTok()
    pump = SessionStreamer(sess, tok, chunk_frames=4)
    st = tok.streams
    assert st.n == 3
    got, done, pumps = {}, set(), 0
    while not sess.idle:
        feeds = st.feeds
        out = pump.pump()
        pumps += 1
        assert st.feeds - feeds <= 1                              # everything pulled goes through ONE feed
        for t, wav, d in out:
            assert t not in done
            got[t] = got.get(t, 0) + wav.shape[2]
            if d:
                done.add(t)
        assert len(pump.ids) <= 3 and len(set(pump.ids.values())) == len(pump.ids)
        assert sorted(list(pump.ids.values()) + pump.free) == [0, 1, 2]
        assert pumps < 500
    assert done == set(lengths) and got == {t: 3 * n for t, n in lengths.items()}
    assert st.max_active <= 3 and not st.active and len(st.resets) == len(lengths) - 3
    assert sorted(t for t, _, _ in pump.take_results()) == sorted(lengths) and pump.take_results() == []
