// thermo_legacy.h -- the `legacy-heuristic` mismatch penalty of ipcr-thermo, one implementation for the host entry
// points (thermo_host.cpp) and the kernel (thermo_kernels.hip).
//
// What it restates (internal/thermovisitors/score.go:363-458 with allowGap either way, :282-297; core/thermo/mismatch.go:86-189;
// mismatch_params.go:46-96; mismatch_triplet_params.go:263-271): a primer P (5'->3', pure ACGT) lies on a target T given
// 3'->5', |P| == |T| == n.  The reference's DP allows one 1-nt gap, but a gap leaves i - j = +-1 and the gap state only moves
// diagonally, so with equal lengths it never reaches dp[n][n]: the result is the left-to-right sum, over the positions i
// where P[i] / T[i] is not a Watson-Crick pair, of mm(i) * w(i), clamped at 0 from below.
//   w(i)  = 2.0 for i >= n - 3, else 1.5 for i < 3, else 1.0 (the 3' test first)
//   mm(i) = ddG * 1000.0 / D for D > 0, else 4.0 (the dTm triplet table is empty, its look-up never succeeds)
//   ddG   = the triplet value when all six bytes are ACGT and both flanks pair (192 contexts), else the pair-family value by
//           (p, t) for t in ACGT, else (t == N) 1.0, less 0.05 when the four flanks hold at least two more G/C than A/T.
// Flanks come from the two strings: outside [0, n) they are N whatever the genome holds there.
//
// Bases are codes: A 0, C 1, G 2, T 3, anything else 4 ("N").  The complement of code c < 4 is 3 - c.
// Everything is float64 *, /, + in this order; both translation units that include this file are compiled with
// -ffp-contract=off, so the device's result equals the host's bit for bit.
//
// Deviation: none in the arithmetic.  On the device a window base is A/C/G/T where the tiles hold an upper-case A/C/G/T and N
// otherwise -- a lower-case base of a record given raw reads as N, which is what the reference's compBase (score.go:307-320)
// makes of it too; records loaded from FASTA are upper-cased by the loader.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#define IPCR_THERMO_HD __host__ __device__ inline
#else
#define IPCR_THERMO_HD inline
#endif

#define IPCR_THERMO_N 4u              // code of every byte that is not an upper-case A/C/G/T
#define IPCR_THERMO_FIXED_DENOM 200.0 // --denom fixed (score.go:1524)
#define IPCR_THERMO_NONE (-1.0)       // table slot of a Watson-Crick centre: no such mismatch

IPCR_THERMO_HD uint32_t ipcr_thermo_code(uint32_t byte) {
    return byte == 'A' ? 0u : byte == 'C' ? 1u : byte == 'G' ? 2u : byte == 'T' ? 3u : IPCR_THERMO_N;
}
IPCR_THERMO_HD uint32_t ipcr_thermo_comp(uint32_t code) { return code < 4u ? 3u - code : IPCR_THERMO_N; } // compBase, score.go:307-320

// ddG (kcal/mol) of the exact triplets, index p5 << 6 | p << 4 | p3 << 2 | t: the target's flanks are the complements of
// the primer's (that is the condition for the entry to apply).  Values: tests/golden/thermo/mismatch_triplet_goldens.golden,
// row by row (tests/test_thermo_legacy.py).
IPCR_THERMO_HD double ipcr_thermo_triplet(uint32_t index) {
    constexpr double X = IPCR_THERMO_NONE;
    constexpr double table[256] = {
        /* p5 p: p3 = A (t = A C G T), p3 = C, p3 = G, p3 = T */
        /* A A */ 3.30, 4.21, 2.88, X, 3.22, 3.79, 2.06, X, 3.32, 3.95, 2.53, X, 3.10, 3.53, 2.04, X,
        /* A C */ 4.58, 5.27, X, 4.28, 4.86, 5.40, X, 4.90, 5.13, 5.64, X, 4.65, 4.37, 5.38, X, 4.09,
        /* A G */ 3.02, X, 2.89, 3.63, 3.29, X, 2.28, 3.64, 3.17, X, 2.88, 3.51, 2.88, X, 2.46, 3.50,
        /* A T */ X, 3.16, 1.96, 2.83, X, 3.53, 2.33, 3.32, X, 3.68, 1.93, 2.90, X, 3.25, 2.66, 3.26,
        /* C A */ 3.57, 4.53, 3.22, X, 3.49, 4.11, 2.40, X, 3.59, 4.27, 2.87, X, 3.37, 3.85, 2.38, X,
        /* C C */ 5.00, 5.04, X, 4.66, 5.28, 5.17, X, 5.28, 5.55, 5.41, X, 5.03, 4.79, 5.15, X, 4.47,
        /* C G */ 4.00, X, 3.80, 3.34, 4.27, X, 3.19, 3.35, 4.15, X, 3.79, 3.22, 3.86, X, 3.37, 3.21,
        /* C T */ X, 3.23, 1.97, 2.42, X, 3.60, 2.34, 2.91, X, 3.75, 1.94, 2.49, X, 3.32, 2.67, 2.85,
        /* G A */ 3.16, 4.44, 2.79, X, 3.08, 4.02, 1.97, X, 3.18, 4.18, 2.44, X, 2.96, 3.76, 1.95, X,
        /* G C */ 5.08, 5.53, X, 5.06, 5.36, 5.66, X, 5.68, 5.63, 5.90, X, 5.43, 4.87, 5.64, X, 4.87,
        /* G G */ 3.04, X, 2.47, 3.56, 3.31, X, 1.86, 3.57, 3.19, X, 2.46, 3.44, 2.90, X, 2.04, 3.43,
        /* G T */ X, 3.97, 1.86, 3.15, X, 4.34, 2.23, 3.64, X, 4.49, 1.83, 3.22, X, 4.06, 2.56, 3.58,
        /* T A */ 2.96, 3.83, 2.74, X, 2.88, 3.41, 1.92, X, 2.98, 3.57, 2.39, X, 2.76, 3.15, 1.90, X,
        /* T C */ 5.00, 4.85, X, 4.47, 5.28, 4.98, X, 5.09, 5.55, 5.22, X, 4.84, 4.79, 4.96, X, 4.28,
        /* T G */ 3.91, X, 3.63, 3.52, 4.18, X, 3.02, 3.53, 4.06, X, 3.62, 3.40, 3.77, X, 3.20, 3.39,
        /* T T */ X, 3.30, 2.35, 2.94, X, 3.67, 2.72, 3.43, X, 3.82, 2.32, 3.01, X, 3.39, 3.05, 3.37,
    };
    return table[index & 255u];
}

// the pair-family ddG by (p, t), index p << 2 | t: wobble 0.60, transition 0.85, A/C 1.10, like with like 1.40, and 1.20
// under the four keys a Watson-Crick centre has (mismatch_params.go:46-66 keys all sixteen)
IPCR_THERMO_HD double ipcr_thermo_pair(uint32_t index) {
    constexpr double table[16] = {
        /* p = A */ 1.40, 1.10, 0.85, 1.20,
        /* p = C */ 1.10, 1.40, 1.20, 0.85,
        /* p = G */ 0.85, 1.20, 1.40, 0.60,
        /* p = T */ 1.20, 0.85, 0.60, 1.40,
    };
    return table[index & 15u];
}

// LookupDeltaG (mismatch.go:108-179) over codes; false where the reference returns ok == false (p not ACGT -- every code is
// "ACGT or N", so isNT(t) holds).  Flanks that are not ACGT are N.
IPCR_THERMO_HD bool ipcr_thermo_ddg(uint32_t p5, uint32_t p, uint32_t p3, uint32_t t5, uint32_t t, uint32_t t3, double *out) {
    if (p >= 4u) return false;
    if (t < 4u) {
        if (p5 < 4u && p3 < 4u && t5 == 3u - p5 && t3 == 3u - p3 && t != 3u - p) {
            *out = ipcr_thermo_triplet(p5 << 6 | p << 4 | p3 << 2 | t);
            return true;
        }
        *out = ipcr_thermo_pair(p << 2 | t);
        return true;
    }
    // t == N: no table keys it; the context heuristic's base 1.0 and its one generic tweak (mismatch.go:126-178)
    const uint32_t f[4] = {p5, p3, t5, t3};
    int gc = 0, at = 0;
    for (int k = 0; k < 4; ++k) {
        gc += (f[k] == 1u || f[k] == 2u) ? 1 : 0;
        at += (f[k] == 0u || f[k] == 3u) ? 1 : 0;
    }
    double base = 1.0;
    if (gc >= at + 2) base -= 0.05;
    *out = base;
    return true;
}

// posMultiplier (score.go:282-290)
IPCR_THERMO_HD double ipcr_thermo_weight(uint32_t i, uint32_t n) {
    if (i + 3u >= n) return 2.0;
    if (i < 3u) return 1.5;
    return 1.0;
}

// one position of the sum: *sum += mm(i) * w(i) when (p, t) is not a Watson-Crick pair
IPCR_THERMO_HD void ipcr_thermo_step(double *sum, uint32_t i, uint32_t n, uint32_t p5, uint32_t p, uint32_t p3, uint32_t t5,
                                     uint32_t t, uint32_t t3, double denom) {
    if (p < 4u && t == 3u - p) return;
    double ddg = 0.0, pen = 4.0; // (4.0: no look-up succeeded, score.go:392-394 -- not reached for an ACGT primer)
    if (ipcr_thermo_ddg(p5, p, p3, t5, t, t3, &ddg)) pen = denom > 0.0 ? (ddg * 1000.0) / denom : 4.0; // DeltaGToDeltaTm
    *sum = *sum + pen * ipcr_thermo_weight(i, n);
}

// "never better than perfect" (score.go:453-457)
IPCR_THERMO_HD double ipcr_thermo_clamp(double sum) { return sum < 0.0 ? 0.0 : sum; }
