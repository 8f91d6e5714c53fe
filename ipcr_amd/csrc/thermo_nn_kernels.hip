// thermo_nn_kernels.hip -- the nn-duplex-v1 score of ipcr-thermo on the device (gfx950).
//
//  thermo_nn_duplex_kernel   per product: its two primer-length windows and the template base next to each primer's 3' end,
//                            read from the tiles, against the product's two primers -> Score = the smaller anneal margin, one
//                            double per product, and -- when asked -- the two ends as ipcr_thermo_nn_end
//
// The arithmetic is thermo_nn.h, shared with the host entry point; this file is compiled with -ffp-contract=off so that
// raw * mult + term and the running sum stay a multiply and adds, as on the host.  The Tm and the denominator of
// a primer's perfect duplex come from the host: nothing here takes a logarithm.
//
// Lanes: as thermo_legacy_kernel -- a lane takes one END (ends 2 i and 2 i + 1 belong to product i: neighbouring lanes of one
// wave, 256 ends = 128 products per workgroup), walks its window base by base in the direction its descriptor gives, three
// dword loads each, and carries the (previous, this, next) codes of primer and target in registers: no per-thread array, no
// LDS.  The even lane takes its neighbour's margin with one shuffle and writes the product's score.
//
// Bounds: the host has checked every window and every dangling position against its record, and every primer index against
// the table, before the launch (host.cpp: thermo_run); this kernel computes no position of its own but P + i / P - i for
// i < n and reads D as given.  The loop is bounded by IPCR_MAX_PRIMER_LEN whatever the descriptor says; table indexes are masked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"
#include "thermo_nn.h"
#include "tile_layout.h"

#define IPCR_THERMO_NN_GROUP 256u    // ends per workgroup
#define IPCR_THERMO_NN_MAX_LEN 128u  // IPCR_MAX_PRIMER_LEN

// code of the base at padded position P (thermo_kernels.hip: thermo_base): the inv plane alone decides what reads N
static __device__ __forceinline__ uint32_t thermo_nn_base(const uint32_t *__restrict__ planes, uint64_t P, bool comp) {
    uint64_t col;
    uint32_t bit, row;
    ipcr_split_pos(P, &col, &bit, &row);
    const uint64_t w = ipcr_plane_word(col >> 6, row, 0, (uint32_t)(col & 63u));
    const uint32_t lo = (planes[w] >> bit) & 1u;
    const uint32_t hi = (planes[w + 256u] >> bit) & 1u;  // next plane: + 64 lanes * 4
    const uint32_t inv = (planes[w + 512u] >> bit) & 1u;
    const uint32_t c = inv ? IPCR_THERMO_N : (lo | (hi << 1));
    return comp ? ipcr_thermo_comp(c) : c;
}

__global__ __launch_bounds__(256) void thermo_nn_duplex_kernel(const uint32_t *__restrict__ planes,
                                                               const ipcr_thermo_nn_end_dev *__restrict__ ends, uint32_t nends,
                                                               const ipcr_thermo_nn_primer_dev *__restrict__ primers, uint32_t nprimers,
                                                               double anneal_c, double *__restrict__ score,
                                                               ipcr_thermo_nn_end *__restrict__ ends_out) {
    const uint32_t e = blockIdx.x * IPCR_THERMO_NN_GROUP + threadIdx.x;
    double margin = __builtin_nan("");
    if (e < nends) {
        const ipcr_thermo_nn_end_dev d = ends[e];
        const uint32_t why = (d.flags >> 8) & 3u; // (the host sets it with n == 0; 1 stands in where a descriptor is not usable)
        ipcr_thermo_nn_end r = ipcr_thermo_nn_unscored(why ? why : 1u);
        if (d.n != 0u && d.primer < nprimers) {
            const ipcr_thermo_nn_primer_dev *__restrict__ pr = primers + d.primer;
            const double denom = pr->denom;
            const uint32_t n = min(min(d.n, pr->len), IPCR_THERMO_NN_MAX_LEN);
            const bool comp = (d.flags & IPCR_THERMO_NN_COMP) != 0u;
            const uint64_t step = (d.flags & IPCR_THERMO_NN_BACK) ? ~0ull : 1ull; // P - i as P + i * (2^64 - 1)
            if (n != 0u) {
                double pen = 0.0;
                uint32_t mismatches = 0, ns = 0;
                uint32_t p5 = IPCR_THERMO_N, t5 = IPCR_THERMO_N;
                uint32_t p = pr->code[0] & 7u, t = thermo_nn_base(planes, d.P, comp);
                for (uint32_t i = 0; i < n; ++i) {
                    const bool more = i + 1u < n; // (the flank behind the window is N even where the genome goes on)
                    const uint32_t p3 = more ? pr->code[i + 1u] & 7u : IPCR_THERMO_N;
                    const uint32_t t3 = more ? thermo_nn_base(planes, d.P + step * (uint64_t)(i + 1u), comp) : IPCR_THERMO_N;
                    ipcr_thermo_nn_step(&pen, &mismatches, &ns, i, n, p5, p, p3, t5, t, t3, denom);
                    p5 = p; p = p3;
                    t5 = t; t = t3;
                }
                // (p5, t5) are the last column now
                const uint32_t x = d.D != IPCR_THERMO_NN_NO_DANGLING ? thermo_nn_base(planes, d.D, comp) : IPCR_THERMO_N;
                r = ipcr_thermo_nn_finish(pen, mismatches, ns, p5, t5, x, pr->tm, denom);
                margin = r.tm_c - anneal_c;
            }
        }
        if (ends_out) ends_out[e] = r;
    }
    // (every lane of the wave comes here: nends is even and so is the group, a product's ends share a wave)
    const double right = __shfl_down(margin, 1, 64);
    if (e < nends && (e & 1u) == 0u) {
        double s = margin; // score.go:683-688: the left margin, the right one when that is smaller
        if (right < s) s = right;
        score[e >> 1] = (margin != margin || right != right) ? __builtin_nan("") : s;
    }
}

namespace ipcr {

hipError_t launch_thermo_nn_duplex(hipStream_t st, const uint32_t *planes, const ipcr_thermo_nn_end_dev *ends, uint32_t nproducts,
                                   const ipcr_thermo_nn_primer_dev *primers, uint32_t nprimers, double anneal_c, double *score,
                                   ipcr_thermo_nn_end *ends_out) {
    if (nproducts == 0) return hipSuccess;
    if (nproducts > 0x40000000u) return hipErrorInvalidValue;
    const uint32_t nends = 2u * nproducts;
    thermo_nn_duplex_kernel<<<dim3((nends + IPCR_THERMO_NN_GROUP - 1u) / IPCR_THERMO_NN_GROUP), dim3(256), 0, st>>>(
        planes, ends, nends, primers, nprimers, anneal_c, score, ends_out);
    return hipGetLastError();
}

} // namespace ipcr
