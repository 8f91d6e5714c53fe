// thermo_nn_host.cpp -- the host-only entry point of the nn-duplex-v1 thermo score: the same thermo_nn.h the kernel runs,
// over strings.  No device is touched.  Compiled with -ffp-contract=off, as thermo_nn_kernels.hip is.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "ipcr_hip.h"
#include "thermo_nn.h"

extern ipcr_status ipcr_internal_fail(ipcr_status st, const char *fmt, ...);

namespace {
uint32_t code_of(char ch) {
    const uint32_t b = (uint8_t)ch;
    return ipcr_thermo_code((b >= 'a' && b <= 'z') ? b - 32u : b);
}
} // namespace

extern "C" {

// ImperfectDuplexWithOptionsAndContext (core/thermo/imperfect.go:248-436) with the default options and ThreePrimeBase =
// dangling3p, the perfect duplex given as (tm_c, denom).  A target byte outside ACGT is N (thermo_nn.h: the one deviation).
ipcr_status ipcr_thermo_nn_duplex_end(const char *primer5to3, const char *target3to5, char dangling3p, double tm_c, double denom,
                                      ipcr_thermo_nn_end *out) {
    if (!primer5to3 || !target3to5 || !out) return ipcr_internal_fail(IPCR_ERR_INVALID, "ipcr_thermo_nn_duplex_end: null argument");
    const size_t n = strlen(primer5to3), m = strlen(target3to5);
    if (n != m || n == 0 || n > IPCR_MAX_PRIMER_LEN)
        return ipcr_internal_fail(IPCR_ERR_INVALID, "ipcr_thermo_nn_duplex_end: primer (%zu) and target (%zu) must have one length of 1 to %d: "
                                  "the model only compares a primer with a window of its own length", n, m, IPCR_MAX_PRIMER_LEN);
    if (!isfinite(tm_c) || !isfinite(denom) || !(denom > 0.0))
        return ipcr_internal_fail(IPCR_ERR_INVALID, "ipcr_thermo_nn_duplex_end: tm_c (%g) must be finite and denom (%g) finite and > 0", tm_c, denom);
    for (size_t i = 0; i < n; ++i)
        if (code_of(primer5to3[i]) >= 4u) {
            *out = ipcr_thermo_nn_unscored(1);
            return IPCR_OK;
        }
    auto P = [&](size_t i) { return i < n ? code_of(primer5to3[i]) : IPCR_THERMO_N; };
    auto T = [&](size_t i) { return i < n ? code_of(target3to5[i]) : IPCR_THERMO_N; };
    double pen = 0.0;
    uint32_t mismatches = 0, ns = 0;
    for (size_t i = 0; i < n; ++i) // (i - 1 wraps to SIZE_MAX at 0: outside [0, n), so N)
        ipcr_thermo_nn_step(&pen, &mismatches, &ns, (uint32_t)i, (uint32_t)n, P(i - 1), P(i), P(i + 1), T(i - 1), T(i), T(i + 1), denom);
    *out = ipcr_thermo_nn_finish(pen, mismatches, ns, P(n - 1), T(n - 1), dangling3p ? code_of(dangling3p) : IPCR_THERMO_N, tm_c, denom);
    return IPCR_OK;
}

} // extern "C"
