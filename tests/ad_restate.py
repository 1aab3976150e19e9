"""``-a auto`` restated in plain Python: the seven sentences of the README section "`-a auto`: the 3' adapter, inferred from the reads",
one function each, on a dictionary of distinct reads with counts.  The yardstick of tests/test_adapter_auto.py (CPU), of the host
build of csrc/kernels_adapter.hpp (tests/test_adapter_auto_hostsim.py) and of the device (tests/test_adapter_auto_gpu.py); no test
in here.  Nothing is shared with the kernels: strings and dicts, no codes, no rolling shift."""
K, P, SPREAD, LEFT_MAX, LEN_MAX = 12, 64, 6, 64, 32
FIELDS = ("seq", "len", "left_steps", "spread", "support", "eligible", "seed_sum", "candidates", "seed", "start")


def eligible(read):
    """sentence 1"""
    return K <= len(read) <= 256 and set(read) <= set("ACGT")


def code(kmer):
    """a k-mer as a number, first letter most significant"""
    v = 0
    for ch in kmer:
        v = 4 * v + "ACGT".index(ch)
    return v


def decode(v, n=K):
    return "".join("ACGT"[(v >> (2 * (n - 1 - q))) & 3] for q in range(n))


def spectrum(reads, counts):
    """sentence 2 -> (T, C, M): C[x] the sum, M[x] the mask of window starts, for every k-mer x some window spells"""
    T, C, M = 0, {}, {}
    for r, c in zip(reads, counts):
        if not eligible(r):
            continue
        T += c
        for p in range(min(len(r) - K, P - 1) + 1):
            x = r[p:p + K]
            C[x] = C.get(x, 0) + c
            M[x] = M.get(x, 0) | (1 << p)
    return T, C, M


def infer(reads, counts):
    """-> dict of FIELDS (every field of ``mirge_adapter``) plus ``C`` and ``M`` (functions of a k-mer string) and ``ties``
    (``{"seed": n, "left": n, "right": n}``: how often the rule for equal C decided)"""
    T, Cd, Md = spectrum(reads, counts)
    C = lambda x: Cd.get(x, 0)
    M = lambda x: Md.get(x, 0)
    spread = lambda x: bin(M(x)).count("1")
    ties = {"seed": 0, "left": 0, "right": 0}
    floor = max(32, -(-T // 20))
    cands = sorted(x for x in Cd if len(set(x)) >= 3 and spread(x) >= SPREAD and C(x) >= floor)  # sentence 3
    out = {"seq": "", "len": 0, "left_steps": 0, "spread": 0, "support": 0, "eligible": T, "seed_sum": 0, "candidates": len(cands),
           "seed": 0, "start": 0, "C": C, "M": M, "ties": ties}
    if not cands:
        return out
    top = max(C(x) for x in cands)  # sentence 4
    best = [x for x in cands if C(x) == top]
    ties["seed"] += len(best) > 1
    seed = best[0]
    first, steps = seed, 0
    for _ in range(LEFT_MAX):  # sentence 5
        ok = [b + first[:K - 1] for b in "ACGT"]
        ok = [y for y in ok if spread(y) >= SPREAD and 10 * C(y) >= 9 * C(first)]
        if not ok:
            break
        top = max(C(y) for y in ok)
        ties["left"] += sum(C(y) == top for y in ok) > 1
        first = [y for y in ok if C(y) == top][0]
        steps += 1
    start = first
    A = start
    while len(A) < LEN_MAX:  # sentence 6
        ok = [A[-K:][1:] + b for b in "ACGT"]
        ok = [z for z in ok if 2 * C(z) >= C(start)]
        if not ok:
            break
        top = max(C(z) for z in ok)
        ties["right"] += sum(C(z) == top for z in ok) > 1
        A += [z for z in ok if C(z) == top][0][-1]
    out.update(seq=A, len=len(A), left_steps=steps, spread=spread(start), support=C(start), seed_sum=C(seed), seed=code(seed),
               start=code(start))  # sentence 7
    return out


def fields(res):
    return {k: res[k] for k in FIELDS}


def probes_of(reads, extra=()):
    """every k-mer of the reads (eligible or not, every window, the ones behind P too) and ``extra`` -> sorted distinct codes"""
    seen = set(extra)
    for r in reads:
        for p in range(len(r) - K + 1):
            x = r[p:p + K]
            if set(x) <= set("ACGT"):
                seen.add(code(x))
    return sorted(seen)


def csv_text(rows):
    """``adapter.auto.csv``: rows of (sample, result of ``infer``, records, distinct)"""
    out = "Sample,Adapter,Length,Support,Eligible,Records,Distinct\n"
    for name, res, records, distinct in rows:
        out += f"{name},{res['seq']},{res['len']},{res['support']},{res['eligible']},{records},{distinct}\n"
    return out


def log_line(name, res, records):
    return f"adapter auto {name}: {res['seq']} (support {res['support']} of {res['eligible']} eligible reads in the first {records} records)"
