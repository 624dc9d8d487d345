"""numpy restatement of the candidate record a sampled vocab-parallel head chains over its lm_head
shards (include/inferd_span.h "Sampled decoding with the vocab-parallel head"; a helper of the
tests, on top of sampling_ref.py, not a test).

    entry   (order(fp32 s) << 32) | (0xFFFFFFFF - global column), s = fp32(logit) / T: one descending
            uint64 key of the order (s descending, column ascending); -0 counts as +0
    record  of a column set X: [count, the first 257 entries of {c in X : s[c] >= v_k(X)} in the
            order, zeros], v_k(X) = the min(top_k, |X|)-th largest s in X; uint64 [258]
    merge   of the records of disjoint X and Y: the same prefix over the union of their entries --
            the record of X | Y, because v_k(X | Y) >= max(v_k(X), v_k(Y)) makes the qualifying columns
            of X | Y that lie in X a prefix of X's own qualifying order, and a 257-prefix of the union's
            order cuts each side within its own first 257
    finish  kept list = the first min(count, 256) entries, overflow iff a 257th exists

Columns whose s is NaN never compare and are left out (the engine makes no bitwise claim there)."""
import numpy as np

import sampling_ref as SR

ENTRIES = 257
WORDS = ENTRIES + 1


def entry_keys(l, T, first_col=0):
    """uint64 entries of the columns of l (fp32 values of bf16 logits, [..., n]); NaN -> 0"""
    s = np.asarray(l, dtype=np.float32) / np.float32(T)
    nan = np.isnan(s)
    s = np.where(s == 0, np.float32(0), s).astype(np.float32)          # -0 -> +0
    u = s.view(np.uint32)
    hi = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    col = (np.uint64(0xFFFFFFFF) - (np.arange(s.shape[-1], dtype=np.uint64) + np.uint64(first_col)))
    keys = (hi << np.uint64(32)) | col
    return np.where(nan, np.uint64(0), keys)


def entry_s(keys):
    h = (np.asarray(keys, dtype=np.uint64) >> np.uint64(32)).astype(np.uint32)
    return np.where(h & np.uint32(0x80000000), h ^ np.uint32(0x80000000), ~h).astype(np.uint32).view(np.float32)


def entry_col(keys):
    return (np.uint64(0xFFFFFFFF) - (np.asarray(keys, dtype=np.uint64) & np.uint64(0xFFFFFFFF))).astype(np.int64)


def _record(keys, k):
    """the record over a set of entries (uint64 1-D, zeros = absent)"""
    keys = keys[keys != 0]
    rec = np.zeros(WORDS, dtype=np.uint64)
    if keys.size == 0:
        return rec
    kk = min(int(k), keys.size)
    if keys.size > 4096:                                    # the kk largest first: O(n)
        top = np.partition(keys, keys.size - kk)[keys.size - kk:]
        keys = keys[keys >= (top.min() >> np.uint64(32) << np.uint64(32))]
    keys = np.sort(keys)[::-1]
    vk = keys[kk - 1] >> np.uint64(32)
    qual = keys[(keys >> np.uint64(32)) >= vk][:ENTRIES]
    rec[0] = qual.size
    rec[1:1 + qual.size] = qual
    return rec


def entries_of(rec):
    return rec[1:1 + int(rec[0])]


def shard_record(keys_row, a, b, k):
    """the record of columns [a, b) of a row's entry keys (entry_keys of the WHOLE row)"""
    return _record(keys_row[a:b], k)


def merge(rec_a, rec_b, k):
    if rec_a is None:
        return rec_b.copy()
    return _record(np.concatenate([entries_of(rec_a), entries_of(rec_b)]), k)


def fold(rec_in, keys_row, a, b, k):
    """what one shard call computes: the record of the columns seen so far plus [a, b)"""
    return merge(rec_in, shard_record(keys_row, a, b, k), k)


def finish(rec):
    """(kept columns in the order, overflow)"""
    n = int(rec[0])
    return entry_col(rec[1:1 + min(n, SR.MAX_KEPT)]), n > SR.MAX_KEPT


def chain(keys_row, bounds, order, k):
    """the records after each shard of `order` (indices into the cuts bounds[i] .. bounds[i + 1])"""
    rec, out = None, []
    for i in order:
        rec = fold(rec, keys_row, bounds[i], bounds[i + 1], k)
        out.append(rec)
    return out


def bounds_of(parts):
    return [0] + [int(v) for v in np.cumsum(parts)]


def cuts(V):
    """the tests' partitions of V columns (multiples of 16): [16, V - 16], two uneven halves, 4 parts
    with one 16-column shard, 8 uneven parts, an empty shard in the middle"""
    t = V // 16
    out = [[16, V - 16]]
    a = max(1, (t * 3) // 8) * 16
    out.append([a, V - a])
    if t >= 4:
        q = max(1, t // 3) * 16
        r = max(1, (t - 1 - q // 16) // 3) * 16
        out.append([q, 16, r, V - q - 16 - r])
    if t >= 8:
        w = np.array([1, 5, 2, 7, 3, 1, 4, 6], dtype=np.float64)
        p = np.maximum(1, np.floor(w / w.sum() * (t - 8)).astype(np.int64) + 1)
        p[-1] += t - int(p.sum())
        out.append([int(v) * 16 for v in p])
    h = max(1, t // 2) * 16
    out.append([h, 0, V - h])
    for c in out:
        assert sum(c) == V and all(v % 16 == 0 and v >= 0 for v in c), c
    return out


def dist_of_record(rec, vocab, p):
    """sampling_ref.RowDist of the finished record: the kept entries' s in a row of -inf, T = 1 and
    top_k = their number reproduce exactly the kept list, then top-p as for any row"""
    cols, overflow = finish(rec)
    row = np.full(vocab, -np.inf, dtype=np.float32)
    row[cols] = entry_s(rec[1:1 + cols.size])
    d = SR.RowDist(row, 1.0, max(1, cols.size), p)
    assert np.array_equal(d.order, cols)
    d.overflow = overflow
    return d


def sample_rows_sharded(logits, bounds, order, T, k, p, seed, positions, row_seeds=None):
    """sampling_ref.sample_rows through the record chain -> (ids, decidable, overflow)"""
    if hasattr(logits, "detach"):
        logits = logits.detach().float().cpu().numpy()
    rows, V = logits.shape
    keys = entry_keys(logits, T)
    rs = list(range(rows)) if row_seeds is None else [int(v) for v in row_seeds]
    ids, dec, ovf = np.zeros(rows, np.int32), np.zeros(rows, bool), np.zeros(rows, bool)
    for r in range(rows):
        d = dist_of_record(chain(keys[r], bounds, order, k)[-1], V, p)
        ids[r], dec[r] = d.draw(SR.uniform(seed, rs[r], int(positions[r])))
        ovf[r] = d.overflow
    return ids, dec, ovf
