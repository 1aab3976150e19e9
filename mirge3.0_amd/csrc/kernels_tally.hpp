// kernels_tally.hpp -- part of mirge_kernels.hpp: k_tally and the member predicate of its lists (k_member_list: kernels_join.hpp).
// Nothing here needs the device: tests/hostsim/tally_sim.cpp compiles this file for the host.
#pragma once

// ------------------------------------------------------------------------------------------
// k_tally (BASELINE config 5): the arithmetic of align2TargetSeq / judgeAllign /
// A2IEditing / mismatchCountAnalysis (mirge/libs/mirge2_tRF_a2i.py:246-518) for every read the cascade annotated to
// a miRNA, against the canonical sequence of that miRNA's FAMILY (the merged name's entry of
// <org>_mirna_SNP_pseudo_<db>.fa, :1037-1044 -- not necessarily the reference the read aligned to).
//   member of its family's list: an exact-miRNA read, or an isomiR read with count * freq[s] >= 1 in some sample
//     (freq[s] = 1e6 / Filtered miRNA Reads, :988-1016);
//   alignment: pairwise2.align.localms(target, read, 2, -1, -20, -20) (:254) = the best-scoring ungapped diagonal
//     (a gap costs 20, more than any annotated read can win back); ties: the alignment that ends first in the
//     target, then first in the read;  d = position of read base 0 relative to target base 0;
//   judgeAllign (:298-332), literally: reject if d > 1; walk the columns from the target's first base to
//     min(end_pos1, end_pos2) (end_pos1 = aligned length - head dashes of the target - 1 - 3, end_pos2 = last read
//     base), count matches and mismatches (a column past the target's end is a mismatch, a column before the read's
//     first base is skipped); accept iff mismatches <= 1 and matches >= Lt - 4 (- 1 more if d == 1);
//   per (family, sample) with count > 0: n_seqs (list length, :1133-1137), and over accepted AND retained reads
//     (retained = the genome filter's answer, :1085-1096): seq_true, count_true, canon (the read is a substring of the
//     target, :350), kept_exact (kept reads that are exact-miRNA rows: checkSeqList, :964-976);
//   census[family][q][target base * 4 + read base][variant][s] for q < Lt - 5 and read base != target base:
//     variant 0 = every member (raw), 1 = accepted, 2 = accepted and retained (mismatchCountAnalysis, :440-517;
//     A -> G of variant 2 is A2IEditing's position count, :358-366).
// The target is one packed word (<= 32 nt).  The read is W = 1 or 2 words: the isomiR policy (-5 1 -3 2 -v 2) annotates
// reads of up to Lt + 3 nt, so a canonical sequence of 29..32 nt has members of 32..35 nt, which sit in the two-word
// group.  Both instances run the same arithmetic: the overlap on a diagonal is at most the target, 32 bases, taken from
// the read with mirge_extract; d >= -(Lr - 1) >= -63 fits the int8 of `diag`.
// ------------------------------------------------------------------------------------------
#define MIRGE_TALLY_MAXPOS 32
struct TallyOut {
    unsigned long long *n_seqs, *seq_true, *count_true, *canon, *kept_exact, *census;
    int8_t *diag, *state;  // per read, handle order: diagonal; 1 accepted / 0 rejected / -1 not a member
};

struct TallyMember {  // a member of its family's list: an exact-miRNA read, or an isomiR read with count * freq[s] >= 1 somewhere
    const int8_t* res_pass; const int32_t* res_ref; const uint32_t* counts; int32_t S, exact_pass, iso_pass;
    const int32_t* fam_of_ref; const double* freq;
    __device__ __forceinline__ bool operator()(uint32_t i) const {
        const int p = res_pass[i];
        if (p != exact_pass && p != iso_pass) return false;
        const int32_t f = fam_of_ref[res_ref[i]];
        bool member = f >= 0 && p == exact_pass;
        if (f >= 0 && p == iso_pass)
            for (int32_t s = 0; s < S; s++) member |= (double)counts[(size_t)i * S + s] * freq[s] >= 1.0;
        return member;
    }
};

template <int W>
__global__ void k_tally(GroupView<W> g, uint32_t base, const uint32_t* __restrict__ orig, const int8_t* __restrict__ res_pass,
                        const int32_t* __restrict__ res_ref, const uint32_t* __restrict__ counts, int32_t S,
                        int32_t exact_pass, int32_t iso_pass, const int32_t* __restrict__ fam_of_ref,
                        const uint64_t* __restrict__ tgt_bits, const uint8_t* __restrict__ tgt_len,
                        const uint8_t* __restrict__ retained, const double* __restrict__ freq, TallyOut o,
                        const uint32_t* __restrict__ list, const uint32_t* __restrict__ n_list, uint32_t chunk) {
    static_assert(W == 1 || W == 2, "k_tally: reads of one or two words");
    const uint32_t n_members = n_list[blockIdx.x];
    for (uint32_t k = threadIdx.x; k < n_members; k += blockDim.x) {
        const uint32_t i = list[(size_t)blockIdx.x * chunk + k];  // a member of its family's list (TallyMember); every other read keeps state -1
        const int p = res_pass[i];
        const uint32_t h = orig ? orig[i] : base + i;
        const int32_t f = fam_of_ref[res_ref[i]];
        const uint64_t tw = tgt_bits[f];
        const int Lt = tgt_len[f], Lr = g.len[i];
        uint64_t rw[W], rn[W];
#pragma unroll
        for (int w = 0; w < W; w++) {
            rw[w] = g.seq[(size_t)w * g.n + i];
            rn[w] = g.nmask ? g.nmask[(size_t)w * g.n + i] : 0ull;
        }
        // ---- best ungapped local alignment: Kadane along every diagonal, +2 / -1
        // (a diagonal whose overlap cannot reach the best score so far is skipped, and the diagonals around the read's
        // own go first so that the bound is tight from the start: ~5-10 of ~55 diagonals are walked for an annotated
        // read.  The update rule is a total order on (score, end in target, end in read): the visiting order is free.
        // Per diagonal the mismatches of the whole overlap come from one XOR of the shifted words, folded to one bit
        // per base, so that the walk itself is 32-bit shifts.)
        int best = 0, best_i = 0, best_j = 0, d = 0;
        const int nd = Lr + Lt - 1;
        for (int k = 0; k < nd + 3; k++) {
            const int dd = k < 3 ? k - 1 : k - 3 - (Lr - 1);  // -1, 0, +1 first, then every diagonal in order
            if (dd <= -Lr || dd >= Lt) continue;
            const int i0 = dd > 0 ? dd : 0, i1 = min(Lt, dd + Lr), j0 = i0 - dd;
            if (2 * (i1 - i0) < best) continue;
            // the read from base j0 on: the overlap is i1 - i0 <= 32 bases of it (what lies above is never walked)
            const uint64_t x = (tw >> (2 * i0)) ^ mirge_extract<W>(rw, j0, 32);
            uint64_t m2 = ((x | (x >> 1)) & 0x5555555555555555ull) | (mirge_extract<W>(rn, j0, 32) & 0x5555555555555555ull);
            m2 = (m2 | (m2 >> 1)) & 0x3333333333333333ull;  // compress the even bits: one mismatch bit per base
            m2 = (m2 | (m2 >> 2)) & 0x0F0F0F0F0F0F0F0Full;
            m2 = (m2 | (m2 >> 4)) & 0x00FF00FF00FF00FFull;
            m2 = (m2 | (m2 >> 8)) & 0x0000FFFF0000FFFFull;
            const uint32_t mis = (uint32_t)(m2 | (m2 >> 16));
            int run = 0;
            for (int t = 0; t < i1 - i0; t++) {
                run = max(0, run + (((mis >> t) & 1u) ? -1 : 2));
                const int ti = i0 + t, rj = j0 + t;
                if (run > best || (run == best && run > 0 && (ti < best_i || (ti == best_i && rj < best_j)))) {
                    best = run; best_i = ti; best_j = rj; d = dd;
                }
            }
        }
        // ---- judgeAllign
        bool state = d <= 1;
        if (state) {
            const int hd_t = d < 0 ? -d : 0, hd_s = d > 0 ? d : 0;
            const int A = max(hd_t + Lt, hd_s + Lr);
            const int last = min(A - hd_t - 1 - 3, hd_s + Lr - 1);
            int mism = 0, match = 0;
            for (int pos = hd_t; pos <= last; pos++) {
                const int rj = pos - hd_s, q = pos - hd_t;
                if (rj < 0) continue;
                const bool eq = q < Lt && !(mirge_extract<W>(rn, rj, 1) & 1ull) && (((tw >> (2 * q)) & 3ull) == mirge_extract<W>(rw, rj, 1));
                if (eq) match++; else mism++;
            }
            state = !(mism > 1 || match < Lt - 3 - 1 - (d == 1 ? 1 : 0));
        }
        o.diag[h] = (int8_t)d;
        o.state[h] = state ? 1 : 0;
        const bool keep = state && (!retained || retained[h]);
        // the read is a substring of the target (`seqList[j] in targetSeq`, :350): any offset, no N (Lr <= Lt: one word)
        bool sub = false;
        if (keep && (rn[0] | rn[W - 1]) == 0ull && Lr <= Lt) {
            const uint64_t m = mirge_lowmask2(Lr);
            for (int a = 0; a + Lr <= Lt && !sub; a++) sub = ((tw >> (2 * a)) & m) == rw[0];
        }
        for (int32_t s = 0; s < S; s++) {
            const unsigned long long c = counts[(size_t)i * S + s];
            if (!c) continue;
            const size_t fs = (size_t)f * S + s;
            atomicAdd(&o.n_seqs[fs], 1ull);
            if (keep) {
                atomicAdd(&o.seq_true[fs], 1ull);
                atomicAdd(&o.count_true[fs], c);
                if (sub) atomicAdd(&o.canon[fs], c);
                if (p == exact_pass) atomicAdd(&o.kept_exact[fs], 1ull);
            }
            for (int q = max(0, d); q < Lt - 5 && q - d < Lr; q++) {
                const int rj = q - d;
                if (mirge_extract<W>(rn, rj, 1) & 1ull) continue;  // an N call is none of the twelve base changes
                const int cb = (int)((tw >> (2 * q)) & 3ull), rb = (int)mirge_extract<W>(rw, rj, 1);
                if (cb == rb) continue;
                unsigned long long* cell = &o.census[((((size_t)f * MIRGE_TALLY_MAXPOS + q) * 16 + cb * 4 + rb) * 3) * S + s];
                atomicAdd(cell, c);
                if (state) atomicAdd(cell + S, c);
                if (keep) atomicAdd(cell + 2 * S, c);
            }
        }
    }
}
