// thermo_kernels.hip -- the legacy-heuristic score of ipcr-thermo on the device (gfx950).
//
//  thermo_legacy_kernel   per product: the two primer-length windows at its ends, read from the tiles, against the
//                         product's two primers -> Score = -(left penalty + right penalty), one double per product
//
// The arithmetic is thermo_legacy.h, shared with the host entry points; this file is compiled with -ffp-contract=off so
// that mm(i) * w(i) and the running sum stay a multiply and an add, as on the host.
//
// Lanes: a lane takes one END (ends 2 i and 2 i + 1 belong to product i, so a product's two ends sit in neighbouring lanes
// of one wave: 256 ends = 128 products per workgroup); it walks its window base by base -- consecutive bases are
// consecutive rows of one tile word column (tile_layout.h), three dword loads each -- and carries the (previous, this,
// next) codes of primer and target in registers: no per-thread array, no table in memory but the two constant ones.  The
// even lane then takes its neighbour's penalty with one shuffle and writes the product's score.  A launch reads at most
// 2 x 128 bases per product scattered over the genome: it is latency- not bandwidth-bound, and the window bytes never
// leave the device.
//
// A window base is A/C/G/T where the tiles hold an upper-case A/C/G/T and N otherwise (the inv plane alone decides: no
// reset plane, no exception runs).  Complemented base by base, not reversed, at both ends (score.go:1529-1547).
// Bounds: the host has checked every window against its record and every primer index against the table before the
// launch (host.cpp: thermo_run); the loop is bounded by IPCR_MAX_PRIMER_LEN whatever the descriptor says.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"
#include "thermo_legacy.h"
#include "tile_layout.h"

#define IPCR_THERMO_GROUP 256u    // ends per workgroup
#define IPCR_THERMO_MAX_LEN 128u  // IPCR_MAX_PRIMER_LEN

// code of the base at padded position P: the addressing of the site read (kernels.hip: base_bits)
static __device__ __forceinline__ uint32_t thermo_base(const uint32_t *__restrict__ planes, uint64_t P) {
    uint64_t col;
    uint32_t bit, row;
    ipcr_split_pos(P, &col, &bit, &row);
    const uint64_t w = ipcr_plane_word(col >> 6, row, 0, (uint32_t)(col & 63u));
    const uint32_t lo = (planes[w] >> bit) & 1u;
    const uint32_t hi = (planes[w + 256u] >> bit) & 1u;  // next plane: + 64 lanes * 4
    const uint32_t inv = (planes[w + 512u] >> bit) & 1u;
    return inv ? IPCR_THERMO_N : (lo | (hi << 1));
}

__global__ __launch_bounds__(256) void thermo_legacy_kernel(const uint32_t *__restrict__ planes,
                                                            const ipcr_thermo_end *__restrict__ ends, uint32_t nends,
                                                            const ipcr_thermo_primer *__restrict__ primers, uint32_t nprimers,
                                                            double *__restrict__ out) {
    const uint32_t e = blockIdx.x * IPCR_THERMO_GROUP + threadIdx.x;
    double pen = 0.0;
    if (e < nends) {
        const ipcr_thermo_end d = ends[e];
        if (d.n != 0u && d.primer < nprimers) {
            const ipcr_thermo_primer *__restrict__ pr = primers + d.primer;
            const double denom = pr->denom;
            const uint32_t n = min(min(d.n, pr->len), IPCR_THERMO_MAX_LEN);
            double sum = 0.0;
            uint32_t p5 = IPCR_THERMO_N, t5 = IPCR_THERMO_N;
            uint32_t p = n ? pr->code[0] : IPCR_THERMO_N, t = n ? ipcr_thermo_comp(thermo_base(planes, d.P)) : IPCR_THERMO_N;
            for (uint32_t i = 0; i < n; ++i) {
                const bool more = i + 1u < n; // (the flank behind the window is N even where the genome goes on)
                const uint32_t p3 = more ? pr->code[i + 1u] : IPCR_THERMO_N;
                const uint32_t t3 = more ? ipcr_thermo_comp(thermo_base(planes, d.P + i + 1u)) : IPCR_THERMO_N;
                ipcr_thermo_step(&sum, i, n, p5, p, p3, t5, t, t3, denom);
                p5 = p; p = p3;
                t5 = t; t = t3;
            }
            pen = ipcr_thermo_clamp(sum);
        }
    }
    // (every lane of the wave comes here: nends is even and so is the group, a product's ends share a wave)
    const double right = __shfl_down(pen, 1, 64);
    if (e < nends && (e & 1u) == 0u) out[e >> 1] = -(pen + right); // pen = 0.0; pen += left; pen += right; Score = -pen
}

namespace ipcr {

hipError_t launch_thermo_legacy(hipStream_t st, const uint32_t *planes, const ipcr_thermo_end *ends, uint32_t nproducts,
                                const ipcr_thermo_primer *primers, uint32_t nprimers, double *out) {
    if (nproducts == 0) return hipSuccess;
    if (nproducts > 0x40000000u) return hipErrorInvalidValue;
    const uint32_t nends = 2u * nproducts;
    thermo_legacy_kernel<<<dim3((nends + IPCR_THERMO_GROUP - 1u) / IPCR_THERMO_GROUP), dim3(256), 0, st>>>(planes, ends, nends, primers,
                                                                                                        nprimers, out);
    return hipGetLastError();
}

} // namespace ipcr
