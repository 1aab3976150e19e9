"""``--umi-cluster directional`` restated in plain Python (no test in here: the UMI tests import it).

The specification is the "directional" network method of UMI-tools (Smith, Heger & Sudbery, Genome Research 2017) on the distinct
UMI-tagged reads of one sample: ``sequential`` is that procedure as published (nodes by descending count, a breadth-first search over the
directed edges from every node not yet found, the searches counted), ``closed_form`` is what the device computes, with founder flags.
``founders`` runs all three -- the sequential search with ties by first appearance and with ties reversed -- and asserts that the molecule
counts agree before it returns the flags, so every input a test uses is checked."""
from collections import deque

MAXLEN = 256


def eligible(t: str, f: int, b: int) -> bool:
    return "N" not in t and len(t) <= MAXLEN and len(t) >= f + b


def umi_positions(n: int, f: int, b: int):
    return list(range(f)) + list(range(n - b, n))


def split(t: str, f: int, b: int):
    """``UMIParser``: (UMI, insert) = (first f + last b letters, the rest)"""
    return t[:f] + (t[len(t) - b:] if b else ""), t[f:len(t) - b]


def neighbours(tagged, f, b):
    """adj[i] = the eligible reads of the same length that differ from eligible read i in exactly one letter, inside the UMI"""
    index = {t: i for i, t in enumerate(tagged) if eligible(t, f, b)}
    assert len(index) == sum(eligible(t, f, b) for t in tagged), "the tagged reads must be distinct"
    adj = [[] for _ in tagged]
    for t, i in index.items():
        for p in umi_positions(len(t), f, b):
            for x in "ACGT":
                if x != t[p]:
                    j = index.get(t[:p] + x + t[p + 1:])
                    if j is not None:
                        adj[i].append(j)
    return index, adj


def sequential(tagged, counts, first, f, b, reverse_ties=False) -> int:
    """UMI-tools' procedure: the number of searches, plus one molecule per ineligible read"""
    index, adj = neighbours(tagged, f, b)
    nodes = sorted(index.values(), key=lambda i: (-int(counts[i]), -int(first[i]) if reverse_ties else int(first[i])))
    found, searches = set(), 0
    for s in nodes:
        if s in found:
            continue
        searches += 1
        found.add(s)
        q = deque([s])
        while q:
            a = q.popleft()
            for v in adj[a]:
                if v not in found and int(counts[a]) >= 2 * int(counts[v]) - 1:
                    found.add(v)
                    q.append(v)
    return searches + (len(tagged) - len(index))


def closed_form(tagged, counts, first, f, b):
    """-> founder flags (list of 0/1, one per tagged read)"""
    index, adj = neighbours(tagged, f, b)
    flags = [1] * len(tagged)
    label = {}
    for i in index.values():
        c = int(counts[i])
        if c >= 2:
            flags[i] = 0 if any(int(counts[a]) >= 2 * c - 1 for a in adj[i]) else 1
        else:
            flags[i] = 0
            label[i] = None
    for s in label:
        if label[s] is not None:
            continue
        comp, q = [s], deque([s])
        label[s] = s
        while q:
            a = q.popleft()
            for v in adj[a]:
                if v in label and label[v] is None:
                    label[v] = s
                    comp.append(v)
                    q.append(v)
        if not any(int(counts[a]) >= 2 for m in comp for a in adj[m]):
            flags[min(comp, key=lambda m: int(first[m]))] = 1
    return flags


def founders(tagged, counts, first, f, b):
    flags = closed_form(tagged, counts, first, f, b)
    n_first = sequential(tagged, counts, first, f, b)
    n_rev = sequential(tagged, counts, first, f, b, reverse_ties=True)
    assert n_first == n_rev == sum(flags), (n_first, n_rev, sum(flags))
    return flags


def insert_counts(tagged, flags, f, b, min_len=0):
    """{insert: founders} over the inserts of at least ``min_len`` letters"""
    out = {}
    for t, fl in zip(tagged, flags):
        ins = split(t, f, b)[1]
        if len(ins) >= min_len:
            out[ins] = out.get(ins, 0) + int(fl)
    return out
