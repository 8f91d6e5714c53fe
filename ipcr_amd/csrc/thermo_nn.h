// thermo_nn.h -- one end of the `nn-duplex-v1` score of ipcr-thermo, one implementation for the host entry point
// (thermo_nn_host.cpp) and the kernel (thermo_nn_kernels.hip).
//
// What it restates (core/thermo/imperfect.go:248-436 with DefaultImperfectDuplexOptions, :451-493; terminal_mismatch_params.go:
// 97-128; dangling_params.go:67-82, :162-176; internal/thermovisitors/score.go:594-690): the imperfect duplex is anchored on the
// primer's own perfect duplex.  Its Tm and its denominator D = |EffectiveDenomCalK| depend on the primer and the solution only;
// they come in as numbers (thermo.panel_nn_base), so nothing here takes a logarithm.  Per site, with the primer P (5'->3',
// pure ACGT) on the target T given 3'->5', |P| == |T| == n:
//   for i = 0 .. n - 1 where P[i] / T[i] is not a Watson-Crick pair, left to right:
//     raw  = ddG * 1000.0 / D                  ddG = ipcr_thermo_ddg (thermo_legacy.h; the dTm triplet table is empty)
//     w    = raw * mult(i) + term(i)           mult = ipcr_thermo_weight; term = 1.5 at i == n - 1, else 0.5 at i == 0, else 0.0
//     pen  = pen + max(w, 0)                   (the clamp cannot act: every ddG is >= 0.60, the N heuristic >= 0.95)
//   pen = max(pen, 0)
//   adj = 0.0 + (-(g * 1000.0) / D)            only when the template base next to the primer's 3' end exists, is A/C/G/T and
//                                              P[n-1] / T[n-1] is a Watson-Crick pair; g = the 5'-dangling dG37 of SantaLucia &
//                                              Hicks 2004 table 3 by (dangling base, T[n-1]).  The primer-5' side gets no term:
//                                              the reference passes ThreePrimeBase only.
//   tm_end = (tm - pen) + adj
// Flanks are N outside [0, n), whatever the genome holds there.  Codes as in thermo_legacy.h (A 0 C 1 G 2 T 3, else 4 = N).
// Everything is float64 *, /, +, - in this order; every translation unit that includes this file is compiled with
// -ffp-contract=off, so the device's result equals the host's bit for bit.
//
// Deviation: a target byte outside ACGT reads as N (the reference errors on one outside ACGTN); on the device that is what
// the inv plane makes of it.
#pragma once
#include <stdint.h>

#include "ipcr_hip.h"
#include "thermo_legacy.h"

// the 5'-dangling dG37 (kcal/mol), index paired << 2 | dangling: `paired` is T[n-1], the template base under the primer's 3'
// end, `dangling` the template base beyond it.  Values: the 5p rows of tests/golden/thermo_nn/dangling_end_goldens.golden.
IPCR_THERMO_HD double ipcr_thermo_nn_dangling(uint32_t index) {
    constexpr double table[16] = {
        /* paired A: X = A C G T */ -0.51, -0.42, -0.62, -0.71,
        /* paired C */ -0.96, -0.52, -0.72, -0.58,
        /* paired G */ -0.58, -0.34, -0.56, -0.61,
        /* paired T */ -0.50, -0.02, 0.48, -0.10,
    };
    return table[index & 15u];
}

// the literal-terminal-base term (imperfect.go:61-62, :326-338): the 3' test first, so n == 1 gives 1.5
IPCR_THERMO_HD double ipcr_thermo_nn_terminal(uint32_t i, uint32_t n) {
    if (i + 1u == n) return 1.5;
    if (i == 0u) return 0.5;
    return 0.0;
}

// one position of the walk: counts a base that reads N; adds the column's term when (p, t) is not a Watson-Crick pair
IPCR_THERMO_HD void ipcr_thermo_nn_step(double *pen, uint32_t *mismatches, uint32_t *ns, uint32_t i, uint32_t n, uint32_t p5,
                                        uint32_t p, uint32_t p3, uint32_t t5, uint32_t t, uint32_t t3, double denom) {
    if (t >= 4u) ++*ns;
    if (p < 4u && t == 3u - p) return;
    double ddg = 0.0, raw = 4.0; // (4.0: DefaultMismatchDeltaTm, no look-up succeeded -- not reached for an ACGT primer)
    if (ipcr_thermo_ddg(p5, p, p3, t5, t, t3, &ddg)) raw = denom > 0.0 ? (ddg * 1000.0) / denom : 4.0; // DeltaGToDeltaTm
    double w = raw * ipcr_thermo_weight(i, n) + ipcr_thermo_nn_terminal(i, n);
    if (w < 0.0) w = 0.0;
    *pen = *pen + w;
    ++*mismatches;
}

// after the walk: p_last / t_last = P[n-1] / T[n-1], dangling = the code of the template base next to the primer's 3' end
// (IPCR_THERMO_N: none, or one that reads N)
IPCR_THERMO_HD ipcr_thermo_nn_end ipcr_thermo_nn_finish(double pen, uint32_t mismatches, uint32_t ns, uint32_t p_last, uint32_t t_last,
                                                        uint32_t dangling, double tm, double denom) {
    if (pen < 0.0) pen = 0.0;
    double adj = 0.0;
    if (dangling < 4u && p_last < 4u && t_last == 3u - p_last) adj = adj + (-(ipcr_thermo_nn_dangling(t_last << 2 | dangling) * 1000.0) / denom);
    ipcr_thermo_nn_end out;
    out.tm_c = (tm - pen) + adj;
    out.mismatch_penalty_c = pen;
    out.dangling_adjustment_c = adj;
    out.mismatch_count = mismatches;
    out.n_count = (uint16_t)ns;
    out.status = 0;
    return out;
}

// an end that is not scored: status 1 (primer not pure ACGT) or 2 (amplicon shorter than the primer); tm_c = NaN
IPCR_THERMO_HD ipcr_thermo_nn_end ipcr_thermo_nn_unscored(uint32_t status) {
    ipcr_thermo_nn_end out;
    out.tm_c = __builtin_nan("");
    out.mismatch_penalty_c = 0.0;
    out.dangling_adjustment_c = 0.0;
    out.mismatch_count = 0;
    out.n_count = 0;
    out.status = (uint16_t)status;
    return out;
}
