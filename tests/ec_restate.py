"""``--kmer-correct`` restated in plain Python: dicts and string slicing, one function per sentence of the specification (README,
"``--kmer-correct``: sequencing errors in reads, by k-mer spectra").  No test in here.  A dictionary is a list of ``(read, count, first index)`` with distinct reads."""

MAXLEN = 256
TALLIES = ("eligible", "suspect", "corrected", "uncorrectable", "unsupported", "ambiguous", "distinct")


def eligible(read, k):
    """1. no N, k <= len <= 256"""
    return "N" not in read and k <= len(read) <= MAXLEN and set(read) <= set("ACGT")


def spectrum(entries, k):
    """2. S_k(x) = sum of c(r) over eligible reads and every window start (forward strand; Python integers do not wrap)"""
    S = {}
    for read, count, _ in entries:
        if eligible(read, k):
            for i in range(len(read) - k + 1):
                x = read[i:i + k]
                S[x] = S.get(x, 0) + count
    return S


def weak_starts(read, k, S, H):
    """3. the weak window starts of an eligible read: S <= H"""
    return [i for i in range(len(read) - k + 1) if S.get(read[i:i + k], 0) <= H]


def candidates(read, k, W):
    """4. lo = max W, hi = min W + k - 1; (p, b) with p in [lo, hi] and [0, len), b != r[p]; p ascending, then A < C < G < T"""
    lo, hi = max(W), min(W) + k - 1
    return [(p, b) for p in range(lo, min(hi, len(read) - 1) + 1) for b in "ACGT" if b != read[p]]


def score(read, k, p, b, S, H):
    """5. the changed read, and the minimum of S over its windows that cover p -- None unless all of them are solid"""
    changed = read[:p] + b + read[p + 1:]
    sums = [S.get(changed[i:i + k], 0) for i in range(max(0, p - k + 1), min(p, len(read) - k) + 1)]
    return changed, (min(sums) if all(s > H for s in sums) else None)


def outcome(read, k, S, H):
    """3.-6. for one eligible read -> (kind, the read it becomes)"""
    W = weak_starts(read, k, S, H)
    if not W:
        return "clean", read
    if max(W) > min(W) + k - 1:
        return "uncorrectable", read
    valid = []
    for p, b in candidates(read, k, W):
        changed, sc = score(read, k, p, b, S, H)
        if sc is not None:
            valid.append((sc, changed))
    if not valid:
        return "unsupported", read
    top = max(sc for sc, _ in valid)
    winners = [changed for sc, changed in valid if sc == top]
    if len(winners) > 1:
        return "ambiguous", read
    return "corrected", winners[0]


def one_round(entries, k, H):
    """one round -> (the regrouped dictionary in first-index order, the successor of every entry, which entries were corrected, the tallies)"""
    S = spectrum(entries, k)
    tally = dict.fromkeys(TALLIES, 0)
    becomes, fixed = [], []
    for read, count, first in entries:
        kind, new = ("ineligible", read)
        if eligible(read, k):
            tally["eligible"] += 1
            kind, new = outcome(read, k, S, H)
            if kind != "clean":
                tally["suspect"] += 1
                tally[kind] += 1
        becomes.append(new)
        fixed.append(kind == "corrected")
    # 7. regroup: counts add, the first index is the minimum
    merged = {}
    for (read, count, first), new in zip(entries, becomes):
        c, f = merged.get(new, (0, first))
        merged[new] = (c + count, min(f, first))
    out = sorted(((s, c, f) for s, (c, f) in merged.items()), key=lambda e: e[2])
    tally["distinct"] = len(out)
    return out, becomes, fixed, tally


def correct(reads, counts, ks, ke, H, first=None):
    """All rounds.  -> dict: ``entries`` (the final dictionary in first-index order), ``final`` (the final read of every input read),
    ``rounds`` (for every input read the k values at which it, or the read it had become, changed), ``tallies`` (one dict per k)."""
    first = list(range(len(reads))) if first is None else list(first)
    entries = sorted(zip(reads, counts, first), key=lambda e: e[2])
    now = list(reads)
    rounds = [[] for _ in reads]
    tallies = []
    for k in range(ks, ke + 1):
        entries_new, becomes, fixed, tally = one_round(entries, k, H)
        step = {e[0]: (new, fx) for e, new, fx in zip(entries, becomes, fixed)}
        for i, r in enumerate(now):
            new, fx = step[r]
            if fx:
                rounds[i].append(k)
            now[i] = new
        entries = entries_new
        tallies.append(tally)
    return {"entries": entries, "final": now, "rounds": rounds, "tallies": tallies}


def csv_text(reads, counts, res):
    """``<sample>_kmerCorrected.csv``: one line per original distinct read whose final sequence differs, in first-appearance order"""
    lines = ["Original,Corrected,Count,Rounds"]
    for r, c, fin, ks in zip(reads, counts, res["final"], res["rounds"]):
        if fin != r:
            lines.append(f"{r},{fin},{int(c)},{';'.join(str(k) for k in ks)}")
    return "\n".join(lines) + "\n"


def log_lines(sample, ks, res):
    return [f"kmer-correct {sample} k={ks + r}: " + ", ".join(f"{name} {t[name]}" for name in TALLIES[:-1]) + f", distinct reads after the round {t['distinct']}"
            for r, t in enumerate(res["tallies"])]
