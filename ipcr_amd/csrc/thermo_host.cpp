// thermo_host.cpp -- the host-only entry points of the legacy-heuristic thermo score: the same thermo_legacy.h the kernel
// runs, over strings.  No device is touched.  Compiled with -ffp-contract=off, as thermo_kernels.hip is.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "ipcr_hip.h"
#include "thermo_legacy.h"

extern ipcr_status ipcr_internal_fail(ipcr_status st, const char *fmt, ...);

namespace {
uint32_t fold(uint32_t b) { return (b >= 'a' && b <= 'z') ? b - 32u : b; }
} // namespace

extern "C" {

// alignPenaltyC_contextualD_ss (score.go:363-458) for |primer| == |target|, single-stranded mode off; the gap switch makes
// no difference there (thermo_legacy.h).  Case is folded as toUpperACGT / toUpperACGTAllowN fold it; a primer with a byte
// outside ACGT, or a target with one outside ACGTN, scores 0.0 as an empty string does (score.go:239-265, :367-369).
ipcr_status ipcr_thermo_legacy_penalty(const char *primer5to3, const char *target3to5, double denom, double *out) {
    if (!primer5to3 || !target3to5 || !out) return ipcr_internal_fail(IPCR_ERR_INVALID, "ipcr_thermo_legacy_penalty: null argument");
    const size_t n = strlen(primer5to3), m = strlen(target3to5);
    *out = 0.0;
    if (n == 0 || m == 0) return IPCR_OK;
    for (size_t i = 0; i < n; ++i)
        if (ipcr_thermo_code(fold((uint8_t)primer5to3[i])) >= 4u) return IPCR_OK;
    for (size_t j = 0; j < m; ++j) {
        const uint32_t b = fold((uint8_t)target3to5[j]);
        if (ipcr_thermo_code(b) >= 4u && b != 'N') return IPCR_OK;
    }
    if (n != m)
        return ipcr_internal_fail(IPCR_ERR_INVALID, "ipcr_thermo_legacy_penalty: primer (%zu) and target (%zu) differ in length: the model "
                                  "only compares a primer with a window of its own length", n, m);
    if (n > 0xFFFFFFFFull) return ipcr_internal_fail(IPCR_ERR_INVALID, "ipcr_thermo_legacy_penalty: string too long");
    auto P = [&](size_t i) { return i < n ? ipcr_thermo_code(fold((uint8_t)primer5to3[i])) : IPCR_THERMO_N; };
    auto T = [&](size_t i) { return i < n ? ipcr_thermo_code(fold((uint8_t)target3to5[i])) : IPCR_THERMO_N; };
    double sum = 0.0;
    for (size_t i = 0; i < n; ++i) // (i - 1 wraps to SIZE_MAX at 0: outside [0, n), so N)
        ipcr_thermo_step(&sum, (uint32_t)i, (uint32_t)n, P(i - 1), P(i), P(i + 1), T(i - 1), T(i), T(i + 1), denom);
    *out = ipcr_thermo_clamp(sum);
    return IPCR_OK;
}

// thermo.LookupDeltaG (core/thermo/mismatch.go:108-179) with the tables as they stand after the package's init; bytes as
// the reference takes them: upper case only.  IPCR_ERR_INVALID where it returns ok == false: p outside ACGT or t outside ACGTN.
ipcr_status ipcr_thermo_mismatch_ddg(char p5, char p, char p3, char t5, char t, char t3, double *out) {
    if (!out) return ipcr_internal_fail(IPCR_ERR_INVALID, "ipcr_thermo_mismatch_ddg: null argument");
    const uint32_t pc = ipcr_thermo_code((uint8_t)p), tc = ipcr_thermo_code((uint8_t)t);
    if (pc >= 4u || (tc >= 4u && t != 'N'))
        return ipcr_internal_fail(IPCR_ERR_INVALID, "ipcr_thermo_mismatch_ddg: no value for primer base 0x%02x against target base 0x%02x",
                                  (unsigned)(uint8_t)p, (unsigned)(uint8_t)t);
    ipcr_thermo_ddg(ipcr_thermo_code((uint8_t)p5), pc, ipcr_thermo_code((uint8_t)p3), ipcr_thermo_code((uint8_t)t5), tc,
                    ipcr_thermo_code((uint8_t)t3), out);
    return IPCR_OK;
}

} // extern "C"
