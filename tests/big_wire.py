"""Expected values for wires longer than 4 GiB and for records placed beyond
4 GiB, without a loop over 4 GiB on the host (tests/test_big_wire_model.py on
the CPU, tests/test_gpu_far_offsets.py and tests/test_gpu_beyond_4gib.py on
the GPU).

Not a test file and not product code. Every operation of the ABI is computed
per record (or per segment) from that record's own bytes, so what it writes
for a record placed somewhere else is what it writes for a small *control*
run, with every value that is a wire position shifted:

  relocate_*   a control output moved by a byte delta: the position fields
               move, everything else stays.
  tile_*       the outputs on  lead | W x P | tail  from the outputs on lead,
               on one block W and on tail, in closed form (control + k |W|,
               counts x P), never by walking the bytes.
  giant_fragments  one extent of L bytes cut at F, as rows.

tests/test_big_wire_model.py pins each of these against the models and the
oracle on a real small concatenation; the GPU tests use nothing else.
"""
from __future__ import annotations

import numpy as np

import onc_rpc_amd.layout as L

LAST = 0x80000000
U64 = np.uint64


# ---------------------------------------------------------------------------
# relocation
# ---------------------------------------------------------------------------
def relocate_offsets(a, delta):
    """rec_off, rec_start, frag_start, frag_off, out_off: all positions."""
    return np.asarray(a, U64) + U64(int(delta))


def position_masks(msgs, status):
    """Which position fields of onc_decoded a decode defines: (payload,
    {cred, verf: (opaque auth, AUTH_UNIX auth)}). An OK call has both auths
    and a payload; an OK accepted reply a verifier, and a payload when it is
    Success; a failed record's descriptor is zero."""
    ok = np.asarray(status) == 0
    call = ok & (msgs["msg_type"] == L.MSG_CALL)
    acc = ok & (msgs["msg_type"] == L.MSG_REPLY) & (msgs["reply_stat"] == L.REPLY_ACCEPTED)
    pay = call | (acc & (msgs["stat"] == L.ACCEPT["success"]))
    auth = {}
    for f, has in (("cred", call), ("verf", call | acc)):
        ux = (msgs[f + "_kind_len"] >> 24) == L.KIND_UNIX
        auth[f] = (has & ~ux, has & ux)
    return pay, auth


def relocate_decoded(dec, delta):
    """(msgs, unix, status, aux0, aux1) of a decode whose wire lies `delta`
    bytes further on: payload_off, the refs of opaque auths and the name_off
    of the AUTH_UNIX slots in use move; slot numbers, statuses and aux stay."""
    msgs, unix, st, a0, a1 = (np.array(x, copy=True) for x in dec[:5])
    d = U64(int(delta))
    pay, auth = position_masks(msgs, st)
    msgs["payload_off"][pay] += d
    for f, (opaque, ux) in auth.items():
        msgs[f + "_ref"][opaque] += d
        unix["name_off"][msgs[f + "_ref"][ux].astype(np.int64)] += d
    return msgs, unix, st, a0, a1


def relocate_pieces(pieces, delta, src=L.PIECE_PAYLOAD):
    """onc_frag_piece rows whose source `src` lies delta bytes further on."""
    p = np.array(pieces, copy=True)
    p["off"][p["src"] == src] += U64(int(delta))
    return p


def relocate_iov(iov, payload=0, wire=0, hdr=0):
    """onc_iov_rec rows: the payload arena, the wire position or the header
    buffer moved."""
    e = np.array(iov, copy=True)
    e["payload_off"][e["payload_len"] > 0] += U64(int(payload))
    e["wire_off"] += U64(int(wire))
    e["hdr_off"] += U64(int(hdr))
    return e


def relocate_seg_rows(rows, first=0):
    """seg_result rows of onc_frame_streams / onc_frame_fragment_streams when
    `first` more records (fragments) precede them: column 0 moves; `consumed`
    and aux count from the segment's own start and stay."""
    r = np.array(rows, U64, copy=True)
    r[:, 0] += U64(int(first))
    return r


# ---------------------------------------------------------------------------
# tiling: lead | W x P | tail
# ---------------------------------------------------------------------------
def tile_offsets(lead, w, P, tail=None):
    """Running offsets (n + 1 entries from 0, the end included) of lead, one
    block and tail -> those of the concatenation. Serves rec_off, frag_off,
    out_off, rec_frag: anything that counts from the start."""
    lead, w = np.asarray(lead, U64), np.asarray(w, U64)
    blocks = w[None, :-1] + (lead[-1] + np.arange(P, dtype=U64) * w[-1])[:, None]
    end = lead[-1] + U64(P) * w[-1]
    rest = np.array([end], U64) if tail is None else np.asarray(tail, U64) + end
    return np.concatenate([lead[:-1], blocks.reshape(-1), rest])


def tile_rows(lead, w, P, tail=None):
    """Per-record values that are no positions (status, rec_len, frag_pre)."""
    parts = [np.asarray(lead), np.tile(np.asarray(w), P)]
    if tail is not None:
        parts.append(np.asarray(tail))
    return np.concatenate(parts)


def pack_unix_slots(msgs, params, status):
    """Descriptors with zeroed AUTH_UNIX refs and each record's (cred, verf)
    parameter blocks (layout.resolve_unix) -> (msgs, unix) in the layout of
    onc_decoded: a 64-record group's OK records put their sets in consecutive
    slots from 128 g."""
    n = len(msgs)
    m = msgs.copy()
    _, auth = position_masks(m, status)
    use = np.stack([auth["cred"][1], auth["verf"][1]], axis=1)             # (n, 2)
    flat = use.reshape(-1).astype(np.int64)
    before = np.cumsum(flat) - flat                                          # sets before this one, overall
    group0 = (np.arange(n) // 64 * 64)
    rank = before.reshape(n, 2) - before[2 * group0][:, None]
    slot = 2 * group0[:, None] + rank
    unix = np.zeros(max(2 * n, 1), L.UNIX_DTYPE)
    ub = unix.view(np.uint8).reshape(-1, L.UNIX_DTYPE.itemsize)
    ub[slot[use]] = params[use]
    m["cred_ref"][use[:, 0]] = slot[:, 0][use[:, 0]].astype(U64)
    m["verf_ref"][use[:, 1]] = slot[:, 1][use[:, 1]].astype(U64)
    return m, unix[:2 * n]


def _moved_and_packed(msgs, params, st, delta):
    """Descriptors with resolved AUTH_UNIX sets (layout.resolve_unix), record
    i's wire delta[i] bytes further on -> (msgs, unix) packed again."""
    pay, auth = position_masks(msgs, st)
    msgs["payload_off"][pay] += delta[pay]
    name_off = params.view(L.UNIX_DTYPE).reshape(-1, 2)["name_off"]
    for k, f in enumerate(("cred", "verf")):
        opaque, ux = auth[f]
        msgs[f + "_ref"][opaque] += delta[opaque]
        name_off[ux, k] += delta[ux]
    return pack_unix_slots(msgs, params, st)


def gather_decoded(dec, idx, delta):
    """Output i = the control's record idx[i] with its wire delta[i] bytes
    further on (onc_decode_extents of moved records in any order): positions
    move per record, and the AUTH_UNIX slots are packed again per 64 outputs."""
    idx = np.asarray(idx, np.int64)
    m, p = L.resolve_unix(*dec[:3])
    st = np.asarray(dec[2])[idx]
    delta = np.broadcast_to(np.asarray(delta, U64), idx.shape)
    msgs, unix = _moved_and_packed(m[idx].copy(), np.ascontiguousarray(p[idx]), st, delta)
    return msgs, unix, st, np.asarray(dec[3])[idx], np.asarray(dec[4])[idx]


def tile_decoded(lead, w, P, lead_len, w_len):
    """The decode of lead | W x P from the decodes of lead and of W, each on
    its own wire from offset 0: block k's positions move by lead_len + k
    w_len, and the AUTH_UNIX slots are packed again per 64 records of the
    whole batch."""
    lm, lp = L.resolve_unix(*lead[:3])
    wm, wp = L.resolve_unix(*w[:3])
    nl, nw = len(lm), len(wm)
    st = tile_rows(lead[2], w[2], P)
    msgs = np.concatenate([lm, np.tile(wm, P)])
    params = np.concatenate([lp, np.tile(wp, (P, 1, 1))])
    delta = np.concatenate([np.zeros(nl, U64),
                            np.repeat(U64(lead_len) + np.arange(P, dtype=U64) * U64(w_len), nw)])
    msgs, unix = _moved_and_packed(msgs, params, st, delta)
    return msgs, unix, st, tile_rows(lead[3], w[3], P), tile_rows(lead[4], w[4], P)


def relocate_by_probe(ctrl, moved, d, delta):
    """For the body-level roots, whose position fields differ per root: the
    oracle's decode at offset 0 (ctrl) and of the same records d bytes further
    on (moved) show which u64 fields are positions (they differ by exactly d);
    those move by delta. -> (msgs, unix, ...rest of ctrl)."""
    msgs, unix = ctrl[0].copy(), ctrl[1].copy()
    for arr, far, names in ((msgs, moved[0], ("payload_off", "cred_ref", "verf_ref")), (unix, moved[1], ("name_off",))):
        for f in names:
            diff = far[f] - arr[f]
            assert np.isin(diff, (0, d)).all(), f
            arr[f][diff == U64(d)] += U64(int(delta))
    return (msgs, unix) + tuple(ctrl[2:])


def relocate_batch(hb, payload=0, auth=0):
    """An encode batch whose payload arena and auth arena lie `payload` and
    `auth` bytes further on in their buffers: payload_off, the refs of opaque
    auths and the names of the AUTH_UNIX table move."""
    msgs, unix = hb.msgs.copy(), hb.unix.copy()
    pay, au = position_masks(msgs, np.zeros(len(msgs), np.int32))
    msgs["payload_off"][pay] += U64(int(payload))
    for f, (opaque, _) in au.items():
        msgs[f + "_ref"][opaque] += U64(int(auth))
    unix["name_off"] += U64(int(auth))
    return msgs, unix


def tile_fragment(lead, w, P):
    """fragment_encode_model.fragment dicts of lead and W -> out_off, status
    and result of onc_fragment on lead | W x P (everything fits)."""
    return {"out_off": tile_offsets(lead["out_off"], w["out_off"], P),
            "status": tile_rows(lead["status"], w["status"], P),
            "result": lead["result"] + U64(P) * w["result"]}


def tile_heads(lead, w, P, lead_nfrag, w_nfrag):
    """heads_model.defragment_heads dicts of the fragments of lead and of W
    (no pending fragments) -> rec_len, rec_frag, frag_pre and status of the
    gather over lead | W x P. frag_pre counts inside a record and stays."""
    lf = np.append(lead["rec_frag"][:len(lead["rec_len"])], U64(lead_nfrag))
    wf = np.append(w["rec_frag"][:len(w["rec_len"])], U64(w_nfrag))
    return {"rec_len": tile_rows(lead["rec_len"], w["rec_len"], P),
            "rec_frag": tile_offsets(lf, wf, P),
            "frag_pre": tile_rows(lead["frag_pre"], w["frag_pre"], P),
            "status": tile_rows(lead["status"], w["status"], P)}


# ---------------------------------------------------------------------------
# one giant extent
# ---------------------------------------------------------------------------
def giant_fragments(length, max_frag):
    """onc_fragment of one extent of `length` >= 4 bytes (its first four are
    its mark) at max_frag: int64 rows (out_pos, src_pos, len, mark): the mark
    at out_pos, then src[src_pos, +len) at out_pos + 4."""
    B, F = int(length) - 4, int(max_frag)
    k = max(1, -(-B // F))
    j = np.arange(k, dtype=np.int64)
    ln = np.minimum(F, B - j * F)
    mark = ln.copy()
    mark[-1] |= LAST
    return np.stack([j * (F + 4), 4 + j * F, ln, mark], axis=1)
