"""numpy restatement of K26 (include/mi355x_match.h, "loop-closure retrieval"): `mi_place_votes` and `mi_place_select` from
np.unpackbits, once as a plain double loop over (query row, database column) -- the semantics as the header words them --
and once vectorised for the larger cases.  Integers throughout; the one float32 multiply of the vote is done in np.float32."""
import numpy as np

F32 = np.float32


def unpack(bits):
    """(..., W) int32 / uint32 -> (..., 32 W) uint8 of 0 / 1 (which bit lands where does not matter to a Hamming distance)"""
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=-1)


def _vote(d1, d2, max_distance, ratio):
    return bool(d1 <= max_distance and F32(d1) < F32(F32(ratio) * F32(d2)))


def frame_loop(db_u, db_valid, q_u, q_valid, num_bits, max_distance, ratio):
    """one query frame against one keyframe, the header's words: (votes, nn_index (Kq), nn_distance (Kq), nn_vote (Kq))"""
    absent = num_bits + 1
    kq, kd = q_u.shape[0], db_u.shape[0]
    nn_i, nn_d, nn_v = np.full(kq, -1, np.int32), np.full(kq, absent, np.int32), np.zeros(kq, bool)
    for i in range(kq):
        if q_valid is not None and not q_valid[i]:
            continue
        keys = sorted((int((q_u[i] != db_u[j]).sum()) << 16) | j for j in range(kd) if db_valid is None or db_valid[j])
        d1, j1 = (keys[0] >> 16, keys[0] & 0xFFFF) if keys else (absent, -1)
        d2 = keys[1] >> 16 if len(keys) > 1 else absent
        nn_i[i], nn_d[i], nn_v[i] = j1, d1, _vote(d1, d2, max_distance, ratio)
    return int(nn_v.sum()), nn_i, nn_d, nn_v


def frame_fast(db_u, db_valid, q_u, q_valid, num_bits, max_distance, ratio):
    """the same, vectorised"""
    absent = num_bits + 1
    kq, kd = q_u.shape[0], db_u.shape[0]
    qf, df = q_u.astype(np.int32), db_u.astype(np.int32)
    ham = qf.sum(1)[:, None] + df.sum(1)[None, :] - 2 * (qf @ df.T)
    key = (ham.astype(np.int64) << 16) | np.arange(kd, dtype=np.int64)[None, :]
    big = np.int64(absent) << 16
    if db_valid is not None:
        key = np.where(np.asarray(db_valid, bool)[None, :], key, big | 0xFFFF)
    key = np.concatenate([key, np.full((kq, 2), big | 0xFFFF, np.int64)], axis=1)       # fewer than two columns
    part = np.sort(key, axis=1)[:, :2]
    d1, d2 = (part[:, 0] >> 16).astype(np.int32), (part[:, 1] >> 16).astype(np.int32)
    j1 = np.where(d1 < absent, part[:, 0] & 0xFFFF, -1).astype(np.int32)
    vote = (d1 <= max_distance) & (d1.astype(F32) < F32(ratio) * d2.astype(F32))
    if q_valid is not None:
        ok = np.asarray(q_valid, bool)
        d1, j1, vote = np.where(ok, d1, absent).astype(np.int32), np.where(ok, j1, -1).astype(np.int32), vote & ok
    return int(vote.sum()), j1, d1, vote


def place_votes(db_bits, db_valid, q_bits, q_valid, max_distance, ratio, frame_index=None, frame=frame_fast):
    """-> (votes (Q, S) int32, nn_index (Q, S, Kq) int32, nn_distance (Q, S, Kq) int32, nn_vote (Q, S, Kq) bool)"""
    db_u, q_u = unpack(db_bits), unpack(q_bits)
    n, q, kq, num_bits = db_u.shape[0], q_u.shape[0], q_u.shape[1], db_u.shape[2]
    index = np.tile(np.arange(n), (q, 1)) if frame_index is None else np.asarray(frame_index)
    s = index.shape[1]
    votes = np.zeros((q, s), np.int32)
    nn_i, nn_d = np.full((q, s, kq), -1, np.int32), np.full((q, s, kq), num_bits + 1, np.int32)
    nn_v = np.zeros((q, s, kq), bool)
    for a in range(q):
        for b in range(s):
            f = int(index[a, b])
            if f < 0:
                continue
            votes[a, b], nn_i[a, b], nn_d[a, b], nn_v[a, b] = frame(
                db_u[f], None if db_valid is None else db_valid[f], q_u[a], None if q_valid is None else q_valid[a], num_bits,
                max_distance, ratio)
    return votes, nn_i, nn_d, nn_v


def place_select(votes, num_candidates, min_votes, excl_lo=None, excl_hi=None):
    """-> (cand_index (Q, C) int32, cand_votes (Q, C) int32)"""
    votes = np.asarray(votes)
    q, n = votes.shape
    ci, cv = np.full((q, num_candidates), -1, np.int32), np.zeros((q, num_candidates), np.int32)
    idx = np.arange(n)
    for a in range(q):
        ok = votes[a] >= min_votes
        if excl_lo is not None:
            ok &= ~((idx >= excl_lo[a]) & (idx < excl_hi[a]))
        cand = idx[ok]
        order = cand[np.lexsort((cand, -votes[a][cand].astype(np.int64)))][:num_candidates]
        ci[a, :len(order)], cv[a, :len(order)] = order, votes[a][order]
    return ci, cv
