// The effective filter and the ring tables of an up-convolution's low-resolution data gradient (ynet_upconv_tables, include/ynet_hip.h; models/ynet.py:463-464).
// Up^T . conv^T over the space-to-depth output gradient is a 3 x 3 convolution with the effective filter
//     Keff[(py, px, co)][ci][a][b] = sum_{ty, tx} M_py[a][ty] K[co][ci][ty][tx] M_px[b][tx]
// plus what the bilinear clamp and the zero padding of the up-sampled image add on the outermost ring (ynet_upconv_dgrad_ring, csrc/glue.hip): 16 tables of the
// same form with dM_s in place of one or both M.  Every value is one bilinear form L^T K R of a 3 x 3 filter tap block with constant 3-vectors L and R: accumulated
// in fp64 without contraction (inner sum over ty, then over tx: the order of the pairwise einsum of ops.upconv_s2d_tables) and rounded to fp32 once.
// A set-up kernel: it runs when the filter version changes (the filter is frozen: the up-convolution has no filter gradient), one thread per output value.
#include "ynet_common.h"

#define UPC_ROW_PAD 16       // the packed layout of ynet_pack_weight (csrc/conv_mfma.hip: YNET_CIN_PAD / YNET_COUT_PAD)
#define UPC_COL_PAD 64

namespace {

// M_p[a][t] (bilinear phase p) and dM_s[p][t] (border side s), include/ynet_hip.h
__device__ __forceinline__ double upc_m(int p, int a, int t) {
    const double m[2][3][3] = {{{0.75, 0.25, 0.0}, {0.25, 0.75, 0.75}, {0.0, 0.0, 0.25}}, {{0.25, 0.0, 0.0}, {0.75, 0.75, 0.25}, {0.0, 0.25, 0.75}}};
    return m[p][a][t];
}
__device__ __forceinline__ double upc_dm(int s, int p, int t) {
    const double m[2][2][3] = {{{-0.25, 0.25, 0.0}, {0.25, 0.0, 0.0}}, {{0.0, 0.0, 0.25}, {0.0, 0.25, -0.25}}};
    return m[s][p][t];
}

// sum_tx (sum_ty L[ty] k[ty][tx]) R[tx]; L = M_py[a] (lv == 0) or dM_{s}[py] (lv == 1), R alike
__device__ double upc_form(const float* __restrict__ k, int py, int lv, int la, int px, int rv, int rb) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int tx = 0; tx < 3; ++tx) {
        double t = 0.0;
        for (int ty = 0; ty < 3; ++ty) t = t + (lv ? upc_dm(la, py, ty) : upc_m(py, la, ty)) * (double)k[ty * 3 + tx];
        acc = acc + t * (rv ? upc_dm(rb, px, tx) : upc_m(px, rb, tx));
    }
    return acc;
}

__global__ __launch_bounds__(256) void upconv_tables_kernel(const float* __restrict__ w, int cout, int cin, float* __restrict__ keff, long long rows_pad,
                                                            long long cols_pad, float* __restrict__ tab) {
    const long long C4 = 4ll * cout, nk = rows_pad * 9 * cols_pad, nt = 16 * C4 * cin;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < nk + nt; i += (long long)gridDim.x * 256) {
        if (i < nk) {      // packed Keff, mode 1 of ynet_pack_weight: [c'][tap][ci] with the taps flipped, zero padding
            const long long m = i % cols_pad, r = i / cols_pad;
            const int tap = (int)(r % 9);
            const long long c = r / 9;
            float v = 0.f;
            if (c < C4 && m < cin) {
                const int ph = (int)(c / cout), co = (int)(c % cout), ab = 8 - tap;
                v = (float)upc_form(w + ((long long)co * cin + m) * 9, ph >> 1, 0, ab / 3, ph & 1, 0, ab % 3);
            }
            keff[i] = v;
        } else {           // tables [16][C4][cin]
            const long long j = i - nk;
            const int ci = (int)(j % cin);
            const long long r = j / cin;
            const int c = (int)(r % C4), q = (int)(r / C4);
            const int ph = c / cout, co = c % cout, py = ph >> 1, px = ph & 1;
            const float* k = w + ((long long)co * cin + ci) * 9;
            double v;
            if (q < 6) v = upc_form(k, py, 1, q / 3, px, 0, q % 3);                     // rows: dM_s[py] K M_px[b]      (q = s * 3 + b)
            else if (q < 12) v = upc_form(k, py, 0, (q - 6) % 3, px, 1, (q - 6) / 3);    // columns: M_py[a] K dM_s[px]  (q = 6 + s * 3 + a)
            else v = upc_form(k, py, 1, (q - 12) >> 1, px, 1, (q - 12) & 1);             // corners: dM_sv[py] K dM_sh[px]  (q = 12 + 2 sv + sh)
            tab[j] = (float)v;
        }
    }
}

}  // namespace

extern "C" {

long long ynet_upconv_tables_floats(int cout, int cin, long long* keff_floats, long long* table_floats) {
    if (cout < 1 || cin < 1 || cout > (1 << 28)) return -1;
    const long long c4 = 4ll * cout;
    const long long k = ((c4 + UPC_ROW_PAD - 1) / UPC_ROW_PAD * UPC_ROW_PAD + UPC_ROW_PAD) * 9 * (((long long)cin + UPC_COL_PAD - 1) / UPC_COL_PAD * UPC_COL_PAD);
    const long long t = 16 * c4 * cin;
    if (keff_floats) *keff_floats = k;
    if (table_floats) *table_floats = t;
    return k + t;
}

int ynet_upconv_tables(const float* w, int cout, int cin, float* keff_packed, float* tables, void* stream) {
    YNET_REQUIRE(w && keff_packed && tables, "upconv_tables: null pointer");
    YNET_REQUIRE(cout >= 1 && cin >= 1 && cout <= (1 << 28), "upconv_tables: bad shape cout %d cin %d", cout, cin);
    const long long c4 = 4ll * cout;
    const long long rows_pad = (c4 + UPC_ROW_PAD - 1) / UPC_ROW_PAD * UPC_ROW_PAD + UPC_ROW_PAD, cols_pad = ((long long)cin + UPC_COL_PAD - 1) / UPC_COL_PAD * UPC_COL_PAD;
    const long long n = rows_pad * 9 * cols_pad + 16 * c4 * cin;
    const long long g = (n + 255) / 256;
    hipLaunchKernelGGL(upconv_tables_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, (hipStream_t)stream, w, cout, cin, keff_packed, rows_pad, cols_pad,
                       tables);
    return ynet_check_launch("upconv_tables");
}

}  // extern "C"
