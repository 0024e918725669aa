"""The device framer (frame.hip: frame_guess, frame_chunks, frame_walk,
frame_write_slots / frame_write) on streams built for its edges, each
compared with the caller's expected_message_len loop (oracle.frame_stream)
on all six outputs: rec_off, n, consumed, status, aux0, aux1.

The streams come from tests/frame_model.py; tests/test_frame_model.py
proves on the CPU that each has the property it is named for (starts per
chunk around kStartsCap, chunk sizes that are no multiple of 16, marks
across chunk boundaries, nested streams whose chunks guess off the chain
and leave stale stop flags, failures over all three levels of the flag
hierarchy, scratch reuse)."""
import time

import numpy as np
import pytest

import frame_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import onc_rpc_amd.runtime as R
    return R


@pytest.fixture(scope="module")
def codec(R):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = R.Codec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def chunk_codec(R, codec):
    """Codecs by (frame_chunk, force_scan), made once; (None, False) is the
    module's default codec."""
    made = {(None, False): codec}

    def get(chunk=None, force_scan=False):
        key = (chunk, force_scan)
        if key not in made:
            made[key] = R.Codec(0, frame_chunk=chunk or 0, force_scan=force_scan)
        return made[key]

    yield get
    for key, c in made.items():
        if key != (None, False):
            c.close()


_oracle_cache = {}


def _frame_both(R, codec, oracle, buf, max_records=None, key=None):
    """The device framing of buf == the oracle's, all six outputs. key: the
    oracle's result is computed once per (key, max_records) and shared."""
    g = R.frame_host_stream(codec, buf, max_records)
    if key is None:
        o = oracle.frame_stream(buf, max_records)
    else:
        k = (key, max_records)
        if k not in _oracle_cache:
            _oracle_cache[k] = oracle.frame_stream(buf, max_records)
        o = _oracle_cache[k]
    assert g[1:] == o[1:], (g[1:], o[1:])
    assert g[0].shape == o[0].shape
    bad = np.nonzero(g[0] != o[0])[0]
    assert len(bad) == 0, f"rec_off differs first at record {bad[0]}: {g[0][bad[:4]]} vs {o[0][bad[:4]]}"
    return o


SCANS = [False, True]


# ---------------------------------------------------------------------------
# (a) starts per chunk around kStartsCap
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("force_scan", SCANS)
@pytest.mark.parametrize("chunk", [1764, 1792, 1820, 1800])
def test_starts_per_chunk_replies(chunk_codec, R, oracle, chunk, force_scan):
    """28-byte Replies, 63 / 64 / 65 (and 64 and 65 mixed) starts in every
    chunk: kept starts copied, or the chunk chased again at the write."""
    buf = M.replies_stream()
    c = chunk_codec(chunk, force_scan)
    o = _frame_both(R, c, oracle, buf, key="replies")
    assert o[1] == 4000 and o[3] == 0
    for m in (63, 64, 65, 64 * 7, 65 * 7 + 1, 3999):
        _frame_both(R, c, oracle, buf, m, key="replies")


@pytest.mark.parametrize("force_scan", SCANS)
@pytest.mark.parametrize("first_len", [4, 8, 12])
def test_starts_per_chunk_opaque_walk(chunk_codec, R, oracle, first_len, force_scan):
    """16-byte opaque records: no chunk guesses, the walk re-chases every
    chunk and keeps its starts itself, 63 / 64 / 65 per chunk."""
    buf = M.opaque16_stream(first_len)
    c = chunk_codec(1024, force_scan)
    o = _frame_both(R, c, oracle, buf, key=("opaque16", first_len))
    assert o[3] == 0 and o[2] == len(buf)
    for m in (64, 65, 66, 129, o[1] - 1):
        _frame_both(R, c, oracle, buf, m, key=("opaque16", first_len))
    _frame_both(R, c, oracle, buf[:-5])


# ---------------------------------------------------------------------------
# (b) chunk sizes that are not multiples of 16; (e)'s nested stream at them
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [65, 100, 1000, 4099])
def test_chunk_not_multiple_of_16(chunk_codec, R, oracle, chunk):
    c = chunk_codec(chunk)
    buf = M.edge_stream()
    o = _frame_both(R, c, oracle, buf, key="edge")
    assert o[1] == 2000 and o[3] == 0
    _frame_both(R, c, oracle, buf[:len(buf) - 7])
    _frame_both(R, c, oracle, buf, 1234, key="edge")
    for variant, gap in ((1, 0), (2, 1), (2, 3), (3, 2)):
        nested = M.nested_stream(1024, 20_000, variant, "first", gap)[0]
        _frame_both(R, c, oracle, nested, key=("nested", 1024, variant, "first", gap))


# ---------------------------------------------------------------------------
# (c) marks straddling chunk boundaries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plausible", "opaque"])
@pytest.mark.parametrize("chunk", [64, 100])
def test_marks_straddling_chunk_boundaries(chunk_codec, R, oracle, chunk, kind):
    buf = M.straddle_stream(chunk, kind)
    c = chunk_codec(chunk)
    o = _frame_both(R, c, oracle, buf)
    assert o[3] == 0 and o[2] == len(buf)
    # and cut inside a straddling mark: IncompleteHeader / IncompleteMessage at a boundary
    ts = M.true_starts(buf)[0]
    for p in ts[(ts % chunk >= chunk - 3) | (ts % chunk <= 1)][-5:]:
        for cut in (int(p) + 1, int(p) + 3, int(p) + 4):
            _frame_both(R, c, oracle, buf[:cut])


# ---------------------------------------------------------------------------
# (d) every max_records and every cut
# ---------------------------------------------------------------------------
def test_every_max_records_and_cut(chunk_codec, R, oracle):
    buf = M.cut_stream()
    c = chunk_codec(64)
    t0 = time.monotonic()
    n = _frame_both(R, c, oracle, buf)[1]
    assert n == 200
    for m in range(0, n + 3):
        _frame_both(R, c, oracle, buf, m)
    cuts = list(range(0, min(len(buf), 700) + 1)) + list(range(len(buf) - 40, len(buf) + 1))
    for cut in cuts:
        _frame_both(R, c, oracle, buf[:cut])
    dt = time.monotonic() - t0
    print(f"every max_records and cut: {n + 3 + len(cuts)} framings in {dt:.2f} s")
    assert dt < 10.0, f"{dt:.1f} s"


# ---------------------------------------------------------------------------
# (e) nested streams and stale flags
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("chunk,inner,variant,placement,gap", M.NESTED_CASES)
def test_nested_stream_stale_flags(chunk_codec, R, oracle, chunk, inner, variant, placement, gap):
    """An outer Call whose payload is a valid stream: the chunks inside it
    guess off the true chain, verify among themselves, and (variants 2, 3:
    the inner stream ends 1, 2 or 3 bytes short) end in a false Fragmented
    stop — flags the walk must leave behind. Both chunk sizes are given to
    the codec explicitly: the preconditions were proved at exactly them."""
    buf, info = M.nested_stream(chunk, inner, variant, placement, gap)
    c = chunk_codec(chunk)
    key = ("nested", chunk, variant, placement, gap)
    o = _frame_both(R, c, oracle, buf, key=key)
    assert o[3] == 0 and o[2] == len(buf)
    k = int(np.searchsorted(o[0], info["outer"]))
    assert o[0][k] == info["outer"] and o[0][k + 1] == info["end"]
    for m in (k, k + 1, k + 2):
        _frame_both(R, c, oracle, buf, m, key=key)
    if chunk == 1024:
        _frame_both(R, chunk_codec(1024, True), oracle, buf, key=key)
    else:
        _frame_both(R, chunk_codec(), oracle, buf, key=key)         # and with the codec's own default chunk


# ---------------------------------------------------------------------------
# (f) flag hierarchy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("force_scan", SCANS)
@pytest.mark.parametrize("name", list(M.HIER_LAYOUTS))
def test_flag_hierarchy(chunk_codec, R, oracle, name, force_scan):
    """More than 2.5 x 65536 chunks; verification failures in three
    different 65536-chunk groups and two 256-chunk groups of one of them, a
    false stop among them, the real stop in the last group."""
    buf, info = M.hier_stream(name)
    o = _frame_both(R, chunk_codec(M.HIER_CHUNK, force_scan), oracle, buf, key=("hier", name))
    assert o[2] == info["stop"] and o[3] == M.FRAGMENTED


# ---------------------------------------------------------------------------
# (g) mark values and tiny buffers
# ---------------------------------------------------------------------------
def test_tiny_buffers_and_marks(chunk_codec, R, oracle):
    for c in (chunk_codec(), chunk_codec(64)):
        for buf in M.tiny_buffers():
            for m in (None, 0, 1, 2):
                _frame_both(R, c, oracle, buf, m)
        o = _frame_both(R, c, oracle, b"\x80\x00\x00\x00")
        assert o[1:4] == (1, 4, 0)
        o = _frame_both(R, c, oracle, b"\x7f\xff\xff\xff")
        assert o[1:4] == (0, 0, M.FRAGMENTED)
        o = _frame_both(R, c, oracle, b"\xff\xff\xff\xff" + b"\x00" * 40)
        assert o[1:] == (0, 0, M.INCOMPLETE_MESSAGE, 44, ((1 << 31) + 3) & 0xFFFFFFFF)


@pytest.mark.parametrize("chunk", [64, 1024])
def test_zero_length_records(chunk_codec, R, oracle, chunk):
    buf = M.zero_records()
    c = chunk_codec(chunk)
    o = _frame_both(R, c, oracle, buf, key="zeros")
    assert o[1:4] == (4000, 16000, 0)
    for m in (1, 16, 17, 256, 257, 3999):
        _frame_both(R, c, oracle, buf, m, key="zeros")
    _frame_both(R, c, oracle, buf[:-1])


# ---------------------------------------------------------------------------
# (h) scratch reuse
# ---------------------------------------------------------------------------
def test_scratch_reuse(R, oracle):
    """One codec frames a large stream, then smaller ones over the same
    scratch (per-chunk state and summary flags of the larger stream behind
    them), the large one again, and larger ones (the second of them needs
    more chunks than the scratch holds: it grows)."""
    c = R.Codec(0, frame_chunk=M.HIER_CHUNK)
    try:
        hier = M.hier_stream("plain")[0]
        _frame_both(R, c, oracle, hier, key=("hier", "plain"))
        small = M.big_filler_stream(100)
        _frame_both(R, c, oracle, small)
        _frame_both(R, c, oracle, M.edge_stream(), key="edge")
        _frame_both(R, c, oracle, M.nested_stream(1024, 20_000, 2, "later", 2)[0],
                    key=("nested", 1024, 2, "later", 2))
        _frame_both(R, c, oracle, hier, key=("hier", "plain"))
        for nbytes in (12 << 20, 17 << 20):
            big = M.big_filler_stream(nbytes)
            o = _frame_both(R, c, oracle, big)
            assert o[2] == len(big) and o[3] == 0
        _frame_both(R, c, oracle, small)
    finally:
        c.close()
