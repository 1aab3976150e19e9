"""``--unmapped-nearest`` restated from the specification (the docstring of mirge3_amd/nearest.py), not from the kernel: a plain column DP.

``nearest(q, hairpins)``: per hairpin the DP with ``D[0][j] = 0`` (any start), a column at a time; row m gives d(q, h) and the smallest end
e >= 1.  A second DP over the reversed strings, anchored at e (``D[0][j] = j``), gives the largest start: the first column j >= 1 whose
row m equals D.  NumPy per column: ``c = min(prev[i-1] + cost, prev[i] + 1)``, then the run of insertions down the column is
``minimum.accumulate(c - i) + i``.  ``lev`` and ``nearest_exhaustive`` are the definition itself, for tests/test_nearest.py."""
import numpy as np

MIN_LEN, MAX_LEN = 12, 64
_ACGT = frozenset("ACGT")


def match(a: str, b: str) -> bool:
    return a == b and a in _ACGT


def _codes(s: str) -> np.ndarray:
    """letters as numbers; a letter that matches nothing gets a number of its own"""
    return np.array(["ACGT".find(ch) if ch in _ACGT else -1 for ch in s], dtype=np.int64)


def _column(prev: np.ndarray, top: int, cost: np.ndarray, ramp: np.ndarray) -> np.ndarray:
    """the next column: prev = D[0..m][j-1], top = D[0][j], cost[i-1] = 0 iff q[i-1] matches the column's letter"""
    c = np.empty_like(prev)
    c[0] = top
    c[1:] = np.minimum(prev[:-1] + cost, prev[1:] + 1)
    return np.minimum.accumulate(c - ramp) + ramp


def _row_m(qc: np.ndarray, hc: np.ndarray, anchored: bool) -> np.ndarray:
    """D[m][j] for j = 0 .. len(h)"""
    m = qc.shape[0]
    ramp = np.arange(m + 1, dtype=np.int64)
    col = ramp.copy()
    out = np.empty(hc.shape[0] + 1, dtype=np.int64)
    out[0] = m
    for j, c in enumerate(hc.tolist(), start=1):
        cost = np.ones(m, dtype=np.int64) if c < 0 else (qc != c).astype(np.int64)
        col = _column(col, j if anchored else 0, cost, ramp)
        out[j] = col[m]
    return out


def nearest(q: str, hairpins):
    """-> (D, hairpin, s, e) by the specification's tie rules, or (-1, -1, -1, -1) for a query outside 12 .. 64 letters or a library
    without a base"""
    if not MIN_LEN <= len(q) <= MAX_LEN:
        return (-1, -1, -1, -1)
    qc = _codes(q)
    best = None
    for k, h in enumerate(hairpins):
        if not h:
            continue
        row = _row_m(qc, _codes(h), False)[1:]
        d = int(row.min())
        if best is None or d < best[0]:
            best = (d, k, int(np.argmax(row == d)) + 1)
    if best is None:
        return (-1, -1, -1, -1)
    D, k, e = best
    back = _row_m(qc[::-1].copy(), _codes(hairpins[k][:e][::-1]), True)[1:]
    j = int(np.argmax(back == D)) + 1
    assert back[j - 1] == D
    return (D, k, e - j, e)


def nearest_all(queries, hairpins):
    """-> int arrays dist, hairpin, start, end"""
    got = np.array([nearest(q, hairpins) for q in queries], dtype=np.int64).reshape(len(queries), 4)
    return dict(dist=got[:, 0], hairpin=got[:, 1], start=got[:, 2], end=got[:, 3])


def _batch_columns(qc: np.ndarray, lens: np.ndarray, text: np.ndarray, anchored: bool):
    """the same column DP for many queries at once: qc [n][M] (rows padded with -2, which equals no letter), text [T] (one text for all)
    or [n][T] (padded with -1); yields (j, D[m][j]) for j = 1 .. T.  The cells below a query's row m are those of a longer query
    and touch nothing above them."""
    n, M = qc.shape
    ramp = np.arange(M + 1, dtype=np.int16)[None, :]  # (16 bits hold every cell: none exceeds the rows plus the columns)
    col = np.repeat(ramp, n, axis=0)
    c = np.empty_like(col)
    for j in range(1, text.shape[-1] + 1):
        t = text[..., j - 1]
        cost = ((qc != (t[:, None] if t.ndim else t)) | ((t[:, None] if t.ndim else t) < 0)).astype(np.int16)
        c[:, 0] = j if anchored else 0
        np.minimum(col[:, :-1] + cost, col[:, 1:] + 1, out=c[:, 1:])
        col = np.minimum.accumulate(c - ramp, axis=1) + ramp
        yield j, col[np.arange(n), lens].astype(np.int64)


def nearest_many(queries, hairpins):
    """``nearest`` for every query, the queries of 12 .. 64 letters side by side in one array per column (for sets of thousands)
    -> int arrays dist, hairpin, start, end"""
    n_all = len(queries)
    out = {k: np.full(n_all, -1, dtype=np.int64) for k in ("dist", "hairpin", "start", "end")}
    idx = np.array([i for i, q in enumerate(queries) if MIN_LEN <= len(q) <= MAX_LEN], dtype=np.int64)
    if not idx.size or not any(hairpins):
        return out
    lens = np.array([len(queries[i]) for i in idx], dtype=np.int64)
    n, M = idx.size, int(lens.max())
    qc = np.full((n, M), -2, dtype=np.int64)
    for r, i in enumerate(idx):
        qc[r, :lens[r]] = _codes(queries[i])
    D = np.full(n, np.iinfo(np.int64).max)
    K, E = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for k, h in enumerate(hairpins):
        if not h:
            continue
        for j, row in _batch_columns(qc, lens, _codes(h), False):
            better = row < D  # hairpins and ends ascend: the first strictly smaller score is the tie rule
            D[better], K[better], E[better] = row[better], k, j
    cols = np.minimum(E, lens + D)  # an anchored match of D edits is at most m + D letters long
    T = int(cols.max())
    text = np.full((n, T), -1, dtype=np.int64)
    for r in range(n):
        text[r, :cols[r]] = _codes(hairpins[K[r]][E[r] - cols[r]:E[r]][::-1])
    rq = np.full((n, M), -2, dtype=np.int64)
    for r in range(n):
        rq[r, :lens[r]] = qc[r, :lens[r]][::-1]
    J = np.zeros(n, np.int64)
    for j, row in _batch_columns(rq, lens, text, True):
        first = (J == 0) & (row == D) & (j <= cols)
        J[first] = j
    assert (J > 0).all()
    out["dist"][idx], out["hairpin"][idx], out["start"][idx], out["end"][idx] = D, K, E - J, E
    return out


def reported(q: str, D: int, K: int) -> bool:
    return D >= 0 and D <= min(K, len(q) // 8)


def lev(a: str, b: str) -> int:
    """the unit-cost edit distance of two strings, letters matching by ``match``"""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, start=1):
        cur = [i]
        for j, y in enumerate(b, start=1):
            cur.append(min(prev[j - 1] + (0 if match(x, y) else 1), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[len(b)]


def nearest_exhaustive(q: str, hairpins, min_len: int = MIN_LEN, max_len: int = MAX_LEN):
    """the definition, over every non-empty substring of every hairpin"""
    if not min_len <= len(q) <= max_len:
        return (-1, -1, -1, -1)
    best = None
    for k, h in enumerate(hairpins):
        for e in range(1, len(h) + 1):
            for s in range(e - 1, -1, -1):
                d = lev(q, h[s:e])
                if best is None or d < best[0]:  # (k, then e ascending, then s descending: the first strictly smaller wins the ties)
                    best = (d, k, s, e)
    return best if best is not None else (-1, -1, -1, -1)
