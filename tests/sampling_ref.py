"""fp64 numpy restatement of the engine's sampled draw (include/inferd_span.h "Sampled decoding";
a helper of the sampling tests, not a test).

    l[c]  fp32 of the row's bf16 logits
    s     = l / T (one fp32 division)
    top-k : v_k = the min(k, V)-th largest s; every column with s >= v_k is kept (ties too), ordered
            by (s descending, column ascending); more than MAX_KEPT: the first MAX_KEPT, overflow
    top-p : q = softmax of the kept s; column j goes iff the sum of q over j and everything after it
            is <= 1 - p; never the first
    draw  : q renormalised; u selects the first column whose running sum exceeds u (none: the last)
    u     = (splitmix64(key + pos) >> 40) * 2^-24, key = splitmix64(splitmix64(seed) + row_seed)

The engine evaluates the softmax and the running sums in fp32; this file in fp64.  DELTA = 2e-5 is
about 20x the fp32 error bound of a 256-term softmax running sum (~1e-6, a hardware exp2 over
|s - max| <= 64 included).  A comparison closer than DELTA is AMBIGUOUS: a top-p tail sum within
DELTA of 1 - p, or u within DELTA of a running-sum boundary.  A case is UNDECIDABLE, and left out of
exact comparisons, when an ambiguous comparison can change the drawn id: u is ambiguous against a
boundary, or the draw differs between removing every column with an ambiguous tail and keeping
every one of them (what stays is a prefix of the order and the boundaries move monotonically with
its length, so every resolution in between then draws the same id too).  Calling a case undecidable
as soon as ANY tail is ambiguous would be the simpler rule, but it throws away every case of a row
that keeps a far softmax tail against top_p = 1 (V = 48 with top_k = 64: tails below 2e-5 against a
threshold of 0, a quarter of that input's cases), although no resolution of it moves a boundary by
more than the tail itself; the rule here compares those cases exactly as well."""
import numpy as np

from oracle import weightgen as wg

DELTA = 2e-5
MAX_K, MAX_KEPT = 64, 256
PARAM_SETS = ((0.6, 20, 0.95), (1.5, 64, 0.5), (1.0, 1, 1.0), (1.0, 64, 1.0))
_M64 = (1 << 64) - 1


def _sm(x: int) -> int:
    return int(wg.splitmix64(np.array([x & _M64], dtype=np.uint64))[0])


def uniform(seed: int, row_seed: int, pos: int) -> np.float32:
    key = _sm(_sm(seed) + row_seed)
    return np.float32((_sm(key + pos) >> 40) * 2.0 ** -24)


def uniforms(seed: int, row_seeds, positions) -> np.ndarray:
    return np.array([uniform(seed, int(r), int(p)) for r, p in zip(row_seeds, positions)], dtype=np.float32)


def bf16_logits(rows: int, vocab: int, gen_seed: int = 1, scale: float = 3.0):
    """The tests' random rows: randn * scale rounded to bf16 (a torch tensor)."""
    import torch
    g = torch.Generator().manual_seed(gen_seed)
    return (torch.randn(rows, vocab, generator=g) * scale).to(torch.bfloat16)


def kept_order(l, T, k, max_kept=MAX_KEPT):
    """(columns kept by temperature + top-k in the order, their s, overflow)"""
    s = np.asarray(l, dtype=np.float32) / np.float32(T)
    V = s.size
    kk = min(int(k), V)
    vk = np.partition(s, V - kk)[V - kk]
    cols = np.nonzero(s >= vk)[0]
    order = cols[np.lexsort((cols, -s[cols].astype(np.float64)))]
    overflow = order.size > max_kept
    order = order[:max_kept]
    return order, s[order].astype(np.float64), overflow


class RowDist:
    """One row's distribution after temperature, top-k and top-p (independent of the draw)."""

    def __init__(self, l, T, k, p, delta=DELTA):
        order, sk, self.overflow = kept_order(l, T, k)
        q = np.exp(sk - sk[0])
        q /= q.sum()
        tail = np.cumsum(q[::-1])[::-1]
        thr = 1.0 - float(np.float32(p))
        removed = tail <= thr
        removed[0] = False
        ambiguous = np.abs(tail - thr) < delta
        ambiguous[0] = False
        self.cut_decidable = not bool(ambiguous.any())    # no tail sum within delta of 1 - p
        m = int(np.count_nonzero(~removed))
        assert not removed[:m].any()          # what stays is a prefix
        # the shortest and the longest prefix an fp32 evaluation may keep
        m_lo = int(np.count_nonzero(~(removed | ambiguous)))
        m_hi = int(np.count_nonzero(~(removed & ~ambiguous)))
        assert 1 <= m_lo <= m <= m_hi and not (removed | ambiguous)[:m_lo].any()
        self.n_topk, self.order, self.kept, self.sk = int(order.size), order, order[:m], sk
        self.probs = q[:m] / q[:m].sum()
        self.cum = np.cumsum(self.probs)
        self._alts = [np.cumsum(q[:mm] / q[:mm].sum()) for mm in sorted({m_lo, m_hi} - {m})]
        self.delta = delta

    @staticmethod
    def _pick(cum, u):
        return min(int(np.searchsorted(cum, u, side="right")), cum.size - 1)      # the first running sum > u

    def draw(self, u):
        """(id, decidable) for the uniform u"""
        u = float(u)
        idx = self._pick(self.cum, u)
        dec = True
        for cum in [self.cum] + self._alts:
            dec = dec and self._pick(cum, u) == idx and not bool(np.any(np.abs(cum[:-1] - u) < self.delta))
        return int(self.kept[idx]), dec


def sample_row(l, T, k, p, u, delta=DELTA):
    """One row's draw: (id, decidable, RowDist)."""
    d = RowDist(l, T, k, p, delta)
    i, dec = d.draw(u)
    return i, dec, d


def sample_rows(logits, T, k, p, seed, positions, row_seeds=None):
    """logits: float array / bf16 torch tensor [rows, V]; positions [rows] or [n_pos, rows] ->
    (ids int32, decidable bool, both shaped like positions; overflow bool [rows])."""
    if hasattr(logits, "detach"):
        logits = logits.detach().float().cpu().numpy()
    rows = logits.shape[0]
    rs = list(range(rows)) if row_seeds is None else [int(v) for v in row_seeds]
    pos = np.asarray(positions)
    pos2 = pos.reshape(-1, rows)
    ids = np.zeros(pos2.shape, dtype=np.int32)
    dec = np.zeros(pos2.shape, dtype=bool)
    ovf = np.zeros(rows, dtype=bool)
    for r in range(rows):
        d = RowDist(logits[r], T, k, p)
        ovf[r] = d.overflow
        for j in range(pos2.shape[0]):
            ids[j, r], dec[j, r] = d.draw(uniform(seed, rs[r], int(pos2[j, r])))
    return ids.reshape(pos.shape), dec.reshape(pos.shape), ovf


def crafted_rows(vocab: int, k: int = 20):
    """Rows that exercise the edges (float32 values exact in bf16), [5, vocab]: one dominant logit
    (kept set of 1 under top-p), an exact tie straddling the k-th value, all-equal logits, the
    maximum in the last tile, the maximum in the first tile."""
    rng = np.random.RandomState(7)
    base = (rng.randn(5, vocab) * 2).astype(np.float32)
    base = (base.view(np.uint32) & 0xFFFF0000).view(np.float32)       # bf16-exact
    base[0, vocab // 3] = 60.0
    top = np.argsort(-base[1])[:k + 4]
    base[1, top[k - 3:k + 4]] = base[1, top[k - 3]]                   # 7 equal values across rank k
    base[2, :] = 1.5
    base[3, vocab - 3] = 30.0
    base[4, 2] = 30.0
    return base
