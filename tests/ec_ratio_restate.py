"""``--kmer-correct --kmer-ratio R`` restated in plain Python, from sentences 2a and 2b of the specification (README, "``--kmer-correct``:
sequencing errors in reads, by k-mer spectra"): a k-mer above H is *dominated* iff a k-mer one letter from it has at least R times its
sum, and a window is weak iff its sum is at most H or its k-mer is dominated.  Sentences 1 and 3-7 are those of tests/ec_restate.py,
with "weak" and "solid" read in this sense; nothing in here sets a sum to zero.  No test in here.  ``R = 0``: no relative threshold."""
import ec_restate
from ec_restate import TALLIES, candidates, eligible, spectrum


def neighbours(x):
    """the 3 k k-mers that differ from x in exactly one letter"""
    return [x[:q] + b + x[q + 1:] for q in range(len(x)) for b in "ACGT" if b != x[q]]


def dominated(S, k, H, R):
    """2a. the k-mers x with S(x) > H for which some y one letter away has S(y) >= R S(x) (Python integers: exact)"""
    if not R:
        return set()
    return {x for x, s in S.items() if s > H and any(S.get(y, 0) >= R * s for y in neighbours(x))}


def weak(x, S, H, dom):
    """2b."""
    return S.get(x, 0) <= H or x in dom


def weak_starts(read, k, S, H, dom):
    """3."""
    return [i for i in range(len(read) - k + 1) if weak(read[i:i + k], S, H, dom)]


def score(read, k, p, b, S, H, dom):
    """5. the changed read and the smallest S over its windows that cover p -- None unless all of them are solid"""
    changed = read[:p] + b + read[p + 1:]
    wins = [changed[i:i + k] for i in range(max(0, p - k + 1), min(p, len(read) - k) + 1)]
    return changed, (None if any(weak(x, S, H, dom) for x in wins) else min(S[x] for x in wins))


def outcome(read, k, S, H, dom):
    """3.-6. for one eligible read -> (kind, the read it becomes)"""
    W = weak_starts(read, k, S, H, dom)
    if not W:
        return "clean", read
    if max(W) > min(W) + k - 1:
        return "uncorrectable", read
    valid = []
    for p, b in candidates(read, k, W):
        changed, sc = score(read, k, p, b, S, H, dom)
        if sc is not None:
            valid.append((sc, changed))
    if not valid:
        return "unsupported", read
    top = max(sc for sc, _ in valid)
    winners = [changed for sc, changed in valid if sc == top]
    if len(winners) > 1:
        return "ambiguous", read
    return "corrected", winners[0]


def one_round(entries, k, H, R):
    """one round -> (the regrouped dictionary in first-index order, the successor of every entry, which entries were corrected, the
    tallies, A = distinct k-mers with S > H, D = the dominated among them)"""
    S = spectrum(entries, k)
    dom = dominated(S, k, H, R)
    tally = dict.fromkeys(TALLIES, 0)
    becomes, fixed = [], []
    for read, count, first in entries:
        kind, new = ("ineligible", read)
        if eligible(read, k):
            tally["eligible"] += 1
            kind, new = outcome(read, k, S, H, dom)
            if kind != "clean":
                tally["suspect"] += 1
                tally[kind] += 1
        becomes.append(new)
        fixed.append(kind == "corrected")
    merged = {}  # 7.
    for (read, count, first), new in zip(entries, becomes):
        c, f = merged.get(new, (0, first))
        merged[new] = (c + count, min(f, first))
    out = sorted(((s, c, f) for s, (c, f) in merged.items()), key=lambda e: e[2])
    tally["distinct"] = len(out)
    return out, becomes, fixed, tally, (sum(1 for s in S.values() if s > H) if R else 0), len(dom)


def correct(reads, counts, ks, ke, H, R, first=None):
    """All rounds -> what ``ec_restate.correct`` returns, plus ``above`` and ``dominated``: one number per round (zeros with R = 0)"""
    first = list(range(len(reads))) if first is None else list(first)
    entries = sorted(zip(reads, counts, first), key=lambda e: e[2])
    now = list(reads)
    rounds = [[] for _ in reads]
    tallies, above, dominated_ = [], [], []
    for k in range(ks, ke + 1):
        entries_new, becomes, fixed, tally, a, d = one_round(entries, k, H, R)
        step = {e[0]: (new, fx) for e, new, fx in zip(entries, becomes, fixed)}
        for i, r in enumerate(now):
            new, fx = step[r]
            if fx:
                rounds[i].append(k)
            now[i] = new
        entries = entries_new
        tallies.append(tally); above.append(a); dominated_.append(d)
    return {"entries": entries, "final": now, "rounds": rounds, "tallies": tallies, "above": above, "dominated": dominated_}


def ratio_log_lines(sample, ks, R, res):
    return [f"kmer-correct {sample} k={ks + r} ratio {R}: k-mers above -kh {a}, dominated {d}" for r, (a, d) in enumerate(zip(res["above"], res["dominated"]))]


def zeroed(S, dom):
    """the spectrum with the dominated sums set to 0 (what the kernels do; the tests assert that it decides every read alike)"""
    return {x: (0 if x in dom else s) for x, s in S.items()}


assert ec_restate.TALLIES is TALLIES
