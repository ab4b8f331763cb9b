// Direct convolution as an implicit GEMM on the gfx950 fp32 matrix cores.
//
// Replaces the ATen conv2d / convolution_backward(dgrad) calls of the reference's Y-Net
// (models/ynet.py:150,192-211,420-451; K1/K2/K3 in SURVEY.md section 2.1).  One kernel serves
//   * forward:  y = [relu](conv(cat(src0,src1,src2), W) + bias)       (fused concat, bias, ReLU)
//   * dgrad:    dx_i = conv(dy * [y > 0], W^T flipped)                (fused ReLU mask, split outputs)
// because dgrad of a stride-1 "same" convolution is a convolution with the flipped, transposed filter;
// the two differ only in the packed filter handed in (see ynet_pack_weight).
//
// Kernels in this file (fp32 MFMA = an exact fmaf chain at the vector-ALU peak, 64 FLOP/clk/SIMD):
//   conv_dma_kernel<NT,R,CC,MASK,X4,FOLD>   3x3, aligned planes: v_mfma_f32_16x16x4_f32, M = 16 pixels, N = 16 output
//       channels (NT tiles per workgroup), K = 4 input channels at one tap; input / filter tiles go global -> LDS
//       by `buffer_load ... lds` (LDS-DMA) into a double buffer, scalar-only control code, buffer stores.
//       The default for every 3x3 launch with >= 2 rows per wave or a folded (W <= 16) map.
//   conv_mfma_kernel<K,NCB,R,CC,MASK,M16>   register-staged generation (global -> VGPR -> LDS): one-row launches
//       of the 32^2..64^2 maps, unaligned planes; 1x1 and 5x5 (M16 = false: the 32x32x2 tile form,
//       M = 32 pixels, N = 32 channels, K = 2 channels).
//   conv1x1_stream_kernel<CT,PX>            the HBM-bound 1x1 predictors (few channels) on the vector ALU.
//   conv_split_reduce_kernel                sums the partials of a channel-split small-map launch (+bias, ReLU).
//   pack_weight_kernel                      checkpoint layout -> packed [cin][tap][cout] (mode 1: flipped/transposed).
// In all of them a lane ends up owning one output channel and 4 consecutive pixels per accumulator quad
// -> 16-byte NCHW stores.  A workgroup = 4 waves computes a 32(x) x 4R(y) pixel tile (folded: 16 x 8R, 8 x 16R)
// for 16*NT (32*NCB) output channels; each wave owns R rows, so one A fragment feeds NT MFMAs and one B
// fragment 2R.  Persistent workgroups walk tiles in an XCD-aware order; 2-4 are resident per CU and overlap
// one group's staging / epilogue with another's MFMAs.  DESIGN.md section 4.1 has the measurements behind
// each choice.
#include "ynet_common.h"
#include <stdlib.h>
#include <stdio.h>

struct ConvArgs {
    YSrc src[YNET_MAX_SRC];
    int nsrc, cin;
    const float* mask;      // optional ReLU mask source (same layout as src[0]); value kept where mask > 0
    long long mask_bs;
    const float* wp;        // packed filter [cin_pad][K*K][cout_pad], zero padded
    const float* bias;      // [cout] or NULL
    YDst dst[YNET_MAX_SRC];
    int ndst;
    int B, H, W, cout, cout_pad, relu;
    int ksplit, cps;        // split of the input-channel chunks over workgroups (small maps): chunks per split
    float* partial;         // [ksplit][B][cout][H][W] raw partial sums when ksplit > 1 (NULL: never split)
    long long partial_cap;  // floats available at `partial`
    const float* addend;    // optional [images][cout][H][W] term added before the ReLU (conv_dma_add_kernel):
    long long addend_bs;    //   y = relu(conv(x) + bias + addend[b % addend_bmod]) -- the part of a convolution over inputs that
    int addend_bmod;        //   repeat along the batch (evaluate()'s K goal samples share the encoder features), computed once
    const float* emask;     // optional [B][cout][H][W] post-ReLU activation whose backward is applied to the OUTPUT (one destination):
    long long emask_bs;     //   dst = emask > 0 ? conv(...) : 0 -- a data gradient written for a consumer that then needs no mask
    int emask_done, pool_done;      //   (host side) emask_done: the launched kernels applied it; pool_done: unused (the plan says so before the launch)
    unsigned* bits_out;     // optional: the epilogue of a ReLU convolution also writes the 1-bit form of its activation mask (y > 0), in the
    const unsigned* bits_in;        //   register layout of its own tiles [tile][256 lanes][WPL words]; bits_in: a data gradient applies such a mask
    int bits_done;                  //   (written by the forward convolution with the SAME output shape, hence the same tiling) instead of emask; bits_done: unused
    float* pool;            // optional second output [B][cout][H/2][W/2] = MaxPool2d(2, 2) of the (post-ReLU) first one, written by
    long long pool_bs;      //   the epilogue (conv_dma_pool_kernel): models/ynet.py:202,215 without the stand-alone pass over y
    int vec_store;          // 16-byte epilogue stores are legal (W % 4 == 0, aligned destinations)
    int vec_load;           // 16-byte LDS-DMA of the input tile is legal (W % 4 == 0, aligned sources / mask)
    int tiles_x, tiles_y, cgroups, ntiles, debug;   // debug: timing ablations only (tools/conv_bench.py)
};

// M16 = false: v_mfma_f32_32x32x2_f32, NCB blocks of 32 output channels per workgroup.
// M16 = true : v_mfma_f32_16x16x4_f32, NCB tiles of 16 output channels (Cout = 16 / 33..48 without padding
//              the N dimension to 32 / 64); same FLOP/clk, pixels in two 16-wide halves.
template <int KS, int NCB, int R, int CC, bool M16 = false>
struct ConvCfg {
    static constexpr int PAD = KS / 2, KK = KS * KS;
    static constexpr int TH = 4 * R, TW = 32;
    static constexpr int TROWS = TH + KS - 1, TCOLS = TW + KS - 1, PLANE = TROWS * TCOLS;
    static constexpr int CB = (M16 ? 16 : 32) * NCB;
    static constexpr int XI = (PLANE + 255) / 256;            // tile elements per thread per channel
    static constexpr int CHS = XI * 256 + (M16 ? 16 : 0);     // LDS channel stride (>= PLANE): unconditional staging stores;
                                                              // = 16 mod 32 for M16 so the 4 channels of a K-step hit distinct banks
    static constexpr int XS_FLOATS = CC * CHS;
    static constexpr int WS_FLOATS = CC * KK * CB;
    static constexpr int LDS_BYTES = (XS_FLOATS + WS_FLOATS) * 4;
};

// Buffer descriptor for one image plane.  The inputs are wave-uniform; readfirstlane makes that
// provable to hipcc, which otherwise wraps every buffer_load in a waterfall loop (guide T20).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(const float* p, unsigned bytes) {
    const unsigned long long u = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    const unsigned nb = __builtin_amdgcn_readfirstlane(p ? bytes : 0u);
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0, nb, 0x00020000);
}

__device__ __forceinline__ float buf_load(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
}

struct TileCoord {
    int ks, cg, x0, y0, b;
};

// Persistent workgroups: each walks tiles blockIdx.x, +gridDim.x, ... and runs ONE software pipeline
// over the flattened (tile, channel-chunk) sequence:
//     [barrier, regs -> LDS, barrier] [issue global loads of the NEXT chunk (maybe of the next tile)]
//     [epilogue stores of the tile that just finished]  [MFMA loop of this chunk]
// so neither a tile's first loads nor its output stores leave the matrix pipes idle.
// accumulator registers per lane: 16 per 32x32 tile, 8 per (16x16 tile x 2 pixel halves)
constexpr int conv_acc_regs(int ncb, int r, bool m16) { return m16 ? 8 * ncb * r : 16 * ncb * r; }
#ifndef YNET_CONV_WAVES_SMALL
#define YNET_CONV_WAVES_SMALL 2     // 3 makes the 64-accumulator variants spill (measured slower)
#endif

template <int KS, int NCB, int R, int CC, bool MASK, bool M16>
__global__ __launch_bounds__(256, (conv_acc_regs(NCB, R, M16) <= 64 ? YNET_CONV_WAVES_SMALL : 2))
void conv_mfma_kernel(const ConvArgs a) {
    using C = ConvCfg<KS, NCB, R, CC, M16>;
    constexpr int PAD = C::PAD, KK = C::KK, TH = C::TH, TW = C::TW;
    constexpr int TCOLS = C::TCOLS, PLANE = C::PLANE, CB = C::CB, CHS = C::CHS;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xs = smem;                  // [CC][CHS] (a TROWS x TCOLS plane per channel)
    float* ws = smem + C::XS_FLOATS;   // [CC][KK][CB]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int HW = __builtin_amdgcn_readfirstlane(a.H * a.W);   // keep plane arithmetic on the scalar unit
    const unsigned plane_bytes = (unsigned)HW * 4u;
    int nchunks = 0;
#pragma unroll
    for (int s = 0; s < YNET_MAX_SRC; ++s)
        if (s < a.nsrc) nchunks += (a.src[s].c + CC - 1) / CC;
    auto item_chunks = [&](const TileCoord& t) { return min(a.cps, nchunks - t.ks * a.cps); };
    // XCD-aware walk: workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8 share an L2), so each
    // XCD gets its own contiguous eighth of the tile space and its 32 CUs sweep neighbouring tiles
    // together: halo rows and filter slices are re-read from that XCD's L2 instead of HBM.
    const bool xcd_walk = (gridDim.x & 7) == 0 && a.ntiles >= (int)gridDim.x && !(a.debug & 32);
    const int per_xcd = (a.ntiles + 7) >> 3;
    const int gstride = xcd_walk ? (int)(gridDim.x >> 3) : (int)gridDim.x;
    const int tile_first = xcd_walk ? (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    const int tile_end = xcd_walk ? min(a.ntiles, ((int)(blockIdx.x & 7) + 1) * per_xcd) : a.ntiles;
    const int ntiles = tile_end;      // exclusive end of this workgroup's tile walk

    auto decode = [&](int t) {
        TileCoord c;
        c.ks = t % a.ksplit;
        t /= a.ksplit;
        c.cg = t % a.cgroups;
        t /= a.cgroups;
        c.x0 = (t % a.tiles_x) * TW;
        t /= a.tiles_x;
        c.y0 = (t % a.tiles_y) * TH;
        c.b = t / a.tiles_y;
        return c;
    };

    f32x16 acc[M16 ? 1 : NCB][M16 ? 1 : R];          // 32x32 accumulators (M16 = false)
    f32x4 acc16[M16 ? NCB : 1][M16 ? R : 1][2];      // 16x16 accumulators: [cout tile][row][pixel half]
    const int r16 = lane & 15, kq = lane >> 4;
    constexpr int XI = C::XI;
    constexpr int ROW4 = CB / 4;
    constexpr int WI = (CC * KK * ROW4 + 255) / 256;       // filter float4 per thread
    float xr[CC][XI], mr[MASK ? CC : 1][MASK ? XI : 1];
    float wr[WI][4];     // (a float4 array is not promoted to registers by hipcc here: scratch)

    // per-thread byte offsets of its XI tile elements inside an image plane (same for every channel
    // and chunk of a tile); out-of-image elements get an offset past the buffer: the hardware range
    // check of buffer_load returns 0 for them, so the staging loop has no branches.
    unsigned goff[XI];
    auto set_goff = [&](const TileCoord& t) {
#pragma unroll
        for (int k = 0; k < XI; ++k) {
            const int i = tid + k * 256;
            const int ty = i / TCOLS, tx = i - ty * TCOLS;
            const int gy = t.y0 + ty - PAD, gx = t.x0 + tx - PAD;
            const bool ok = i < PLANE && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            goff[k] = ok ? (unsigned)(gy * a.W + gx) * 4u : 0x80000000u;    // + channel offsets stays past any buffer
        }
    };

    // Chunks are aligned to the sources of the (virtual) concatenation: chunk j covers up to CC
    // consecutive channels of ONE source, so a chunk needs one buffer descriptor (built from scalars
    // once) and per-channel plane offsets are a vector add; channels past the source's end fall outside
    // the descriptor and read 0 (their filter rows then multiply zeros).
    struct Chunk {
        const float* base;   // plane of the chunk's first channel in image b
        int cnt, cglob;      // valid channels; index of the first one in the concatenation (filter row)
    };
    auto locate = [&](int b, int j) {
        Chunk c{nullptr, 0, 0};
        int start = 0;
#pragma unroll
        for (int s = 0; s < YNET_MAX_SRC; ++s) {
            if (c.base == nullptr && s < a.nsrc) {
                const int n = (a.src[s].c + CC - 1) / CC;
                if (j < n) {
                    c.cnt = min(CC, a.src[s].c - j * CC);
                    c.cglob = start + j * CC;
                    c.base = a.src[s].p + (long long)(a.src[s].bmod > 0 ? b % a.src[s].bmod : b) * a.src[s].bs + (long long)(j * CC) * HW;
                } else {
                    j -= n;
                    start += a.src[s].c;
                }
            }
        }
        return c;
    };
    auto load_chunk = [&](const TileCoord& t, int j) {
        const Chunk ck = locate(t.b, j);
        const __amdgpu_buffer_rsrc_t rx = plane_rsrc(ck.base, (unsigned)ck.cnt * plane_bytes);
        __amdgpu_buffer_rsrc_t rm = rx;
        if (MASK) rm = plane_rsrc(a.mask + (long long)t.b * a.mask_bs + (long long)ck.cglob * HW, (unsigned)ck.cnt * plane_bytes);
#pragma unroll
        for (int c = 0; c < CC; ++c) {
#pragma unroll
            for (int k = 0; k < XI; ++k) {
                const unsigned off = goff[k] + (unsigned)c * plane_bytes;
                xr[c][k] = buf_load(rx, off);
                if (MASK) mr[MASK ? c : 0][MASK ? k : 0] = buf_load(rm, off);
            }
        }
        const int c0 = ck.cglob;
        const float* wsrc = a.wp + (long long)c0 * KK * a.cout_pad + t.cg * CB;
#pragma unroll
        for (int k = 0; k < WI; ++k) {
            int i = tid + k * 256;
            i = i < CC * KK * ROW4 ? i : CC * KK * ROW4 - 1;      // clamp (keeps wr[] in registers)
            const int row = i / ROW4, j4 = i - row * ROW4;
            const float4 v4 = *reinterpret_cast<const float4*>(wsrc + (long long)row * a.cout_pad + j4 * 4);
            wr[k][0] = v4.x;
            wr[k][1] = v4.y;
            wr[k][2] = v4.z;
            wr[k][3] = v4.w;
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int c = 0; c < CC; ++c)
#pragma unroll
            for (int k = 0; k < XI; ++k) {
                const int i = tid + k * 256;
                xs[c * CHS + i] = (!MASK || mr[MASK ? c : 0][MASK ? k : 0] > 0.f) ? xr[c][k] : 0.f;
            }
#pragma unroll
        for (int k = 0; k < WI; ++k) {
            const int i = tid + k * 256;
            if (i < CC * KK * ROW4) reinterpret_cast<float4*>(ws)[i] = make_float4(wr[k][0], wr[k][1], wr[k][2], wr[k][3]);
        }
    };

    // MFMA over (channel pair, tap) of the chunk in LDS.  Operands of tap t+1 are read from LDS while
    // the MFMAs of tap t run (explicit two-stage register pipeline; sched_group_barrier pins "reads
    // first, then MFMAs" so that no MFMA waits on an LDS read issued just before it).
    auto mfma_chunk = [&](int rem) {      // rem = valid channels of the chunk in LDS
        if constexpr (M16) {
            // K = 4 input channels per instruction: lane (r16, kq) feeds pixel r16 (+16 for the second half)
            // of channel kq as A and output channel r16 of channel kq as B.
            const int ngroups = rem >= CC ? CC / 4 : (rem + 3) / 4;
            const float* xb = xs + kq * CHS + (wave * R) * TCOLS + r16;
            const float* wb = ws + kq * KK * CB + r16;
            float a_cur[R][2], b_cur[NCB], a_nxt[R][2], b_nxt[NCB];
#pragma unroll
            for (int i = 0; i < NCB; ++i) b_cur[i] = wb[i * 16];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                a_cur[r][0] = xb[r * TCOLS];
                a_cur[r][1] = xb[r * TCOLS + 16];
            }
#pragma unroll 1
            for (int g = 0; g < ngroups; ++g) {
                const float* xp = xb + 4 * g * CHS;
                const float* wq = wb + 4 * g * KK * CB;
#pragma unroll
                for (int t = 0; t < KK; ++t) {
                    const int tn = (t + 1) % KK;
                    const float* xn = t + 1 < KK ? xp : xp + 4 * CHS;
                    const float* wn = t + 1 < KK ? wq : wq + 4 * KK * CB;
                    const int kyn = tn / KS, kxn = tn % KS;
                    if (t + 1 < KK || g + 1 < ngroups) {
#pragma unroll
                        for (int i = 0; i < NCB; ++i) b_nxt[i] = wn[tn * CB + i * 16];
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            a_nxt[r][0] = xn[(r + kyn) * TCOLS + kxn];
                            a_nxt[r][1] = xn[(r + kyn) * TCOLS + kxn + 16];
                        }
                    }
                    __builtin_amdgcn_sched_group_barrier(0x100, NCB + 2 * R, 0);
#pragma unroll
                    for (int r = 0; r < R; ++r)
#pragma unroll
                        for (int i = 0; i < NCB; ++i) {
                            acc16[i][r][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[r][0], b_cur[i], acc16[i][r][0], 0, 0, 0);
                            acc16[i][r][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[r][1], b_cur[i], acc16[i][r][1], 0, 0, 0);
                        }
                    __builtin_amdgcn_sched_group_barrier(0x8, 2 * NCB * R, 0);
#pragma unroll
                    for (int i = 0; i < NCB; ++i) b_cur[i] = b_nxt[i];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        a_cur[r][0] = a_nxt[r][0];
                        a_cur[r][1] = a_nxt[r][1];
                    }
                }
            }
        } else {
        const int npairs = rem >= CC ? CC / 2 : (rem + 1) / 2;
        const float* xb = xs + half * CHS + (wave * R) * TCOLS + l31;
        const float* wb = ws + half * KK * CB + l31;
        float a_cur[NCB], b_cur[R], a_nxt[NCB], b_nxt[R];
#pragma unroll
        for (int i = 0; i < NCB; ++i) a_cur[i] = wb[i * 32];
#pragma unroll
        for (int r = 0; r < R; ++r) b_cur[r] = xb[r * TCOLS];
#pragma unroll 1
        for (int p = 0; p < npairs; ++p) {
            const float* xp = xb + 2 * p * CHS;
            const float* wq = wb + 2 * p * KK * CB;
#pragma unroll
            for (int t = 0; t < KK; ++t) {
                const int tn = (t + 1) % KK;                     // next tap (of the next pair when t is the last)
                const float* xn = t + 1 < KK ? xp : xp + 2 * CHS;
                const float* wn = t + 1 < KK ? wq : wq + 2 * KK * CB;
                const int kyn = tn / KS, kxn = tn % KS;
                if (t + 1 < KK || p + 1 < npairs) {
#pragma unroll
                    for (int i = 0; i < NCB; ++i) a_nxt[i] = wn[tn * CB + i * 32];
#pragma unroll
                    for (int r = 0; r < R; ++r) b_nxt[r] = xn[(r + kyn) * TCOLS + kxn];
                }
                __builtin_amdgcn_sched_group_barrier(0x100, NCB + R, 0);
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int i = 0; i < NCB; ++i)
                        acc[i][r] = __builtin_amdgcn_mfma_f32_32x32x2f32(b_cur[r], a_cur[i], acc[i][r], 0, 0, 0);
                __builtin_amdgcn_sched_group_barrier(0x8, NCB * R, 0);
#pragma unroll
                for (int i = 0; i < NCB; ++i) a_cur[i] = a_nxt[i];
#pragma unroll
                for (int r = 0; r < R; ++r) b_cur[r] = b_nxt[r];
            }
        }
        }
    };

    // Epilogue: bias, ReLU, scatter to the (possibly split) destination.  D = pixels x cout: lane
    // (l31, half) owns output channel l31 of the block and, in registers 4g..4g+3, the four consecutive
    // pixels x0 + 8g + 4*half .. +3  ->  one 16-byte store each.
    const int d0 = a.dst[0].c, d1 = d0 + (a.ndst > 1 ? a.dst[1].c : 0), d2 = d1 + (a.ndst > 2 ? a.dst[2].c : 0);
    float bias_r[NCB];       // bias of the finished tile's channels, fetched when the tile completes
    auto load_bias = [&](const TileCoord& t) {
#pragma unroll
        for (int i = 0; i < NCB; ++i) {
            const int co = M16 ? t.cg * CB + i * 16 + r16 : t.cg * CB + i * 32 + l31;
            bias_r[i] = (a.bias != nullptr && co < a.cout) ? a.bias[co] : 0.f;
        }
    };
    auto epilogue = [&](const TileCoord& t) {
        // Touch the bias registers unconditionally first: the wait for their (long finished) load is
        // then placed once here and not, as vmcnt(0), in front of every predicated store group below,
        // where it would also wait for the stores already issued.
#pragma unroll
        for (int i = 0; i < NCB; ++i) asm volatile("" : "+v"(bias_r[i]));
#pragma unroll
        for (int i = 0; i < NCB; ++i) {
            const int co = M16 ? t.cg * CB + i * 16 + r16 : t.cg * CB + i * 32 + l31;
            float* dp = nullptr;
            if (a.ksplit > 1) {
                if (co < a.cout) dp = a.partial + (((long long)t.ks * a.B + t.b) * a.cout + co) * HW;
            } else if (co < a.cout) {
                if (co < d0 || a.ndst == 1) {
                    if (a.dst[0].p) dp = a.dst[0].p + (long long)t.b * a.dst[0].bs + (long long)co * HW;
                } else if (co < d1 || a.ndst == 2) {
                    if (a.dst[1].p) dp = a.dst[1].p + (long long)t.b * a.dst[1].bs + (long long)(co - d0) * HW;
                } else if (co < d2 || a.ndst == 3) {
                    if (a.dst[2].p) dp = a.dst[2].p + (long long)t.b * a.dst[2].bs + (long long)(co - d1) * HW;
                } else {
                    if (a.dst[3].p) dp = a.dst[3].p + (long long)t.b * a.dst[3].bs + (long long)(co - d2) * HW;
                }
            }
            if (dp == nullptr) continue;
            const float bsv = a.ksplit > 1 ? 0.f : bias_r[i];
            const bool relu = a.relu && a.ksplit == 1;
            // register quad g of row r holds 4 consecutive pixels starting at px(g)
            constexpr int NG = M16 ? 2 : 4;
            if (a.vec_store) {      // uniform: W % 4 == 0 and every destination plane is 16-byte aligned
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int gy = t.y0 + wave * R + r;
#pragma unroll
                    for (int g = 0; g < NG; ++g) {
                        const int gx = M16 ? t.x0 + 16 * g + 4 * kq : t.x0 + 8 * g + 4 * half;
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float u = (M16 ? acc16[M16 ? i : 0][M16 ? r : 0][g & 1][e] : acc[M16 ? 0 : i][M16 ? 0 : r][(4 * g + e) & 15]) + bsv;
                            if (relu) u = u < 0.f ? 0.f : u;
                            v[e] = u;
                        }
                        if (gy < a.H && gx < a.W)
                            *reinterpret_cast<f32x4*>(__builtin_assume_aligned(dp + (long long)gy * a.W + gx, 16)) = v;
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int gy = t.y0 + wave * R + r;
#pragma unroll
                    for (int g = 0; g < NG; ++g) {
                        const int gx = M16 ? t.x0 + 16 * g + 4 * kq : t.x0 + 8 * g + 4 * half;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float u = (M16 ? acc16[M16 ? i : 0][M16 ? r : 0][g & 1][e] : acc[M16 ? 0 : i][M16 ? 0 : r][(4 * g + e) & 15]) + bsv;
                            if (relu) u = u < 0.f ? 0.f : u;
                            if (gy < a.H && gx + e < a.W) dp[(long long)gy * a.W + gx + e] = u;
                        }
                    }
                }
            }
        }
    };

    // ---- load cursor (lt, lch) runs one chunk ahead of the compute cursor (ct, cch)
    int lt_idx = tile_first, lch = 0;
    if (lt_idx >= ntiles) return;
    TileCoord lt = decode(lt_idx);
    set_goff(lt);
    int lcnt = item_chunks(lt);
    auto advance_load = [&]() {
        if (++lch == lcnt) {
            lch = 0;
            lt_idx += gstride;
            if (lt_idx < ntiles) {
                lt = decode(lt_idx);
                lcnt = item_chunks(lt);
                set_goff(lt);
            }
        }
    };
    load_chunk(lt, lt.ks * a.cps);
    advance_load();

    int ct_idx = tile_first, cch = 0;
    TileCoord ct = decode(ct_idx), pt = ct;
    int ccnt = item_chunks(ct);
    bool pending = false;
    for (;;) {
        const bool have = ct_idx < ntiles;
        const bool stage = have && !((a.debug & 1) && !(ct_idx == tile_first && cch == 0));
        if (stage) {
            if (!(a.debug & 4)) __syncthreads();            // every wave finished reading the previous chunk
            if (!(a.debug & 8)) store_chunk();
            if (!(a.debug & 4)) __syncthreads();
        }
        if (pending) {                  // stores of the finished tile go out before the next prefetch is queued
            if (!(a.debug & 2)) epilogue(pt);
            pending = false;
        }
        if (stage && lt_idx < ntiles) {
            if (!(a.debug & 16)) load_chunk(lt, lt.ks * a.cps + lch);
            advance_load();
        }
        if (!have) break;
        if (cch == 0) {
            if constexpr (M16) {
#pragma unroll
                for (int i = 0; i < NCB; ++i)
#pragma unroll
                    for (int r = 0; r < R; ++r)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc16[i][r][0][q] = acc16[i][r][1][q] = 0.f;
            } else {
#pragma unroll
                for (int i = 0; i < NCB; ++i)
#pragma unroll
                    for (int r = 0; r < R; ++r)
#pragma unroll
                        for (int q = 0; q < 16; ++q) acc[i][r][q] = 0.f;
            }
        }
        mfma_chunk(locate(ct.b, ct.ks * a.cps + cch).cnt);
        if (++cch == ccnt) {
            cch = 0;
            pending = true;
            pt = ct;
            load_bias(pt);
            ct_idx += gstride;
            if (ct_idx < ntiles) {
                ct = decode(ct_idx);
                ccnt = item_chunks(ct);
            }
        }
    }
}

// ================================================================================================
// LDS-DMA generation of the 3x3 kernel (v_mfma_f32_16x16x4_f32 tiles only).
// Staging no longer passes through registers: every thread issues `buffer_load_dword ... lds` (input
// tile, optional ReLU-mask tile) and `buffer_load_dwordx4 ... lds` (filter slice) straight into the
// OTHER half of a double-buffered LDS image while the MFMA loop reads this half; the hardware range
// check writes the zero padding.  Per chunk: one `s_waitcnt vmcnt(0)` + ONE barrier, no ds_write, and
// ~60 fewer VGPRs than the register-staged pipeline.  The ReLU mask of a dgrad is applied when the A
// operand is read (second LDS read + v_cndmask) because a DMA cannot be modified in flight.
// ================================================================================================
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// 16 bytes per lane, global -> LDS (lane i lands at lds + 16 i).  Kept in a __device__ helper: used directly
// inside `if constexpr` in the kernel template, hipcc's host pass silently drops the kernel's stub.
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, const float* lds, unsigned byte_off) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)lds, 16, byte_off, 0, 0, 0);
}

// X4 = true: the input tile is fetched as aligned 16-byte quads, 10 per row ([x0-4, x0+36): W % 4 == 0 makes
// every quad lie wholly inside or wholly outside the image), a quarter of the DMA instructions of the
// dword form for 18 % more bytes; tile column 0 (gx = x0-1) then sits at LDS column 3.
// FOLD = 2 / 4 (feature maps no wider than 16 / 8): the 32 pixels of an MFMA row unit are FOLD rows of
// 32 / FOLD columns instead of one row of 32 (which would compute 50 / 75 % padding); needs H % FOLD == 0.
template <int NCB, int R, int CC, bool MASK, bool X4, int FOLD = 1>
struct DmaCfg {
    static constexpr int KS = 3, PAD = 1, KK = 9;
    static constexpr int TW = 32 / FOLD, TH = 4 * R * FOLD;
    static constexpr int TROWS = TH + 2, TCOLS = X4 ? TW + 8 : TW + 2, PLANE = TROWS * TCOLS;
    static constexpr int XOFF = X4 ? 3 : 0;
    static constexpr int GOFF = FOLD == 1 ? 16 : (16 / TW) * TCOLS;     // LDS distance of the second 16-pixel group
    static constexpr int CB = 16 * NCB;
    static constexpr int XN = X4 ? PLANE / 4 : PLANE;         // DMA lanes per channel
    static constexpr int XI = (XN + 255) / 256;
    // channel stride: the 4 channels of a K-step on distinct banks for the 32 lanes of a ds_read_b32 group
    // (= 16 mod 32 when the 16 pixel lanes are consecutive floats; = 8 mod 32 for FOLD 4: two rows of 8, 16 apart)
    static constexpr int CHS = X4 ? PLANE + (FOLD == 4 ? ((8 - PLANE % 32) + 32) % 32 : 0) : XI * 256 + 16;
    static constexpr int XS_FLOATS = CC * CHS;                // one buffer of the input (or mask) tile
    static constexpr int WS_FLOATS = CC * KK * CB;            // one buffer of the filter slice
    static constexpr int BUF_FLOATS = XS_FLOATS * ((MASK && !X4) ? 2 : 1) + WS_FLOATS;     // (X4: the mask quads stay in registers)
    static constexpr int LDS_BYTES = 2 * BUF_FLOATS * 4;
    // FLAT (the deep-chunk small tiles, CC >= 8): the CC * CHS / 4 quads of a chunk's tile image are ONE flat list of DMA items dealt
    // round-robin to the 256 threads (item q = tid + 256 k lands at LDS quad q; its channel q / (CHS / 4) goes into the per-lane
    // offset), so every wave issues the same CC * CHS / 1024 instructions per chunk.  Without it the lanes tid < PLANE / 4 issue
    // one instruction per channel -- for a folded tile (60 / 72 quads per channel) ALL of them in wave 0, a serial issue stream of
    // CC x ~130 cycles per chunk in front of that wave's MFMAs (round 4; the large tiles keep the per-channel form).
    static constexpr bool FLAT = X4 && CC >= 8;
    static constexpr int XNP = CHS / 4;                       // quads per channel in LDS (the tile's quads + pad)
    static constexpr int NITEM = CC * XNP;
    static constexpr int FI = FLAT ? (NITEM + 255) / 256 : 1;
    static_assert(FOLD == 1 || X4, "folded tiles use the quad layout");
    static_assert(!X4 || (CHS % 32 == (FOLD == 4 ? 8 : 16) && CHS % 4 == 0 && XI == 1), "X4 tile geometry");
};

// Kernel arguments re-read through an opaque pointer to the kernarg segment: the loads are issued (s_load) where
// they are written instead of being hoisted to the kernel entry and kept in SGPRs for its whole life.  With
// every ConvArgs field live the kernel needs > 102 SGPRs and hipcc spills them to VGPR lanes (v_readlane /
// v_writelane); a vector-ALU instruction of a wave whose SIMD neighbours stream MFMAs waits for ~1 MFMA slot
// per neighbour (tools/valu_under_mfma.hip: 38 / 70 / 100 cycles per VALU op with 1 / 2 / 3 MFMA waves on the
// SIMD, 0.8 cycles per SALU op regardless), so the control code of this kernel is written to stay scalar.
typedef const __attribute__((address_space(4))) ConvArgs* conv_kargs_t;
__device__ __forceinline__ conv_kargs_t conv_kargs() {
    conv_kargs_t p = (conv_kargs_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void dma16s(__amdgpu_buffer_rsrc_t r, unsigned lds_byte, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)(uintptr_t)lds_byte, 16, voff, soff, 0, 0);
}
__device__ __forceinline__ void dma4s(__amdgpu_buffer_rsrc_t r, unsigned lds_byte, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)(uintptr_t)lds_byte, 4, voff, soff, 0, 0);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sgpr_rsrc(const void* p, unsigned bytes) {     // p, bytes: scalar values
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, p ? bytes : 0u, 0x00020000);
}

// EPI: 0 plain epilogue, 1 + the batch-shared additive term (ConvArgs::addend), 2 ReLU backward on the output (ConvArgs::emask),
//      3 + the 2 x 2 max-pooled copy of the output (ConvArgs::pool), 4 + the 1-bit activation mask of the (post-ReLU) output
//      (ConvArgs::bits_out), 5 ReLU backward on the output from such a bit mask (ConvArgs::bits_in)
// Bit masks (EPI 4 / 5): a lane's NCB * R * 8 accumulator elements in the order j = ((i * R + r) * 2 + g) * 4 + e are pushed MSB-first
// into WPL = ceil(NCB * R * 8 / 32) words: 8 bytes per lane and tile instead of NCB * R * 2 16-byte quads of activations, fetched with the
// tile's first DMA (like the bias) -- the float form (EPI 2) waits for up to 64 registers of activation quads in its epilogue.
template <int NCB, int R>
struct BitsCfg {
    static constexpr int N = NCB * R * 8, WPL = (N + 31) / 32;
    static constexpr int count(int w) { return N - 32 * w < 32 ? N - 32 * w : 32; }      // elements pushed into word w
};
template <int NCB, int R, int CC, bool MASK, bool X4, int FOLD, int EPI>
__device__ __forceinline__ void conv_dma_body() {
    using C = DmaCfg<NCB, R, CC, MASK, X4, FOLD>;
    constexpr int KS = 3, PAD = 1, KK = 9, TH = C::TH, TW = C::TW;
    constexpr int TCOLS = C::TCOLS, PLANE = C::PLANE, CB = C::CB, CHS = C::CHS, XI = C::XI;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // buffer b: [xs | ms (MASK) | ws]
    auto xs_of = [&](int b) { return smem + b * C::BUF_FLOATS; };
    auto ms_of = [&](int b) { return smem + b * C::BUF_FLOATS + C::XS_FLOATS; };
    auto ws_of = [&](int b) { return smem + b * C::BUF_FLOATS + C::XS_FLOATS * ((MASK && !X4) ? 2 : 1); };
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)smem);     // byte address of the LDS image

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kq = lane >> 4;
    const conv_kargs_t ka = conv_kargs();
    const int H = ka->H, W = ka->W;
    const int HW = H * W;
    const unsigned plane_bytes = (unsigned)HW * 4u;
    const int ksplit = ka->ksplit, cps = ka->cps, cgroups = ka->cgroups, tiles_x = ka->tiles_x, tiles_y = ka->tiles_y;
    const int nsrc = ka->nsrc;
    const unsigned wrow_bytes = (unsigned)ka->cout_pad * 4u;

    const bool xcd_walk = (gridDim.x & 7) == 0 && ka->ntiles >= (int)gridDim.x;
    const int per_xcd = (ka->ntiles + 7) >> 3;
    const int gstride = xcd_walk ? (int)(gridDim.x >> 3) : (int)gridDim.x;
    const int tile_first = xcd_walk ? (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    const int ntiles = xcd_walk ? min(ka->ntiles, ((int)(blockIdx.x & 7) + 1) * per_xcd) : ka->ntiles;
    int nchunks = 0;
#pragma unroll
    for (int s = 0; s < YNET_MAX_SRC; ++s)
        if (s < nsrc) nchunks += (ka->src[s].c + CC - 1) / CC;
    auto item_chunks = [&](const TileCoord& t) { return min(cps, nchunks - t.ks * cps); };
    auto decode = [&](int t) {
        TileCoord c;
        c.ks = t % ksplit;
        t /= ksplit;
        c.cg = t % cgroups;
        t /= cgroups;
        c.x0 = (t % tiles_x) * TW;
        t /= tiles_x;
        c.y0 = (t % tiles_y) * TH;
        c.b = t / tiles_y;
        return c;
    };

    // A workgroup's tiles are gstride apart: their (split, channel group, x, y, image) coordinates advance by a
    // fixed mixed-radix step with carries (scalar adds / compares).  decode() divides -- ~20 vector-ALU
    // instructions per division -- and is only used for the first tile.
    int st_ks, st_cg, st_x, st_y, st_b;
    {
        int q = gstride;
        st_ks = q % ksplit;
        q /= ksplit;
        st_cg = q % cgroups;
        q /= cgroups;
        st_x = q % tiles_x;
        q /= tiles_x;
        st_y = q % tiles_y;
        st_b = q / tiles_y;
    }
    auto advance_tile = [&](TileCoord& c) {
        int carry;
        c.ks += st_ks;
        carry = c.ks >= ksplit ? 1 : 0;
        c.ks -= carry * ksplit;
        c.cg += st_cg + carry;
        carry = c.cg >= cgroups ? 1 : 0;
        c.cg -= carry * cgroups;
        int tx = c.x0 / TW + st_x + carry;          // (TW, TH: powers of two -> shifts)
        carry = tx >= tiles_x ? 1 : 0;
        tx -= carry * tiles_x;
        c.x0 = tx * TW;
        int ty = c.y0 / TH + st_y + carry;
        carry = ty >= tiles_y ? 1 : 0;
        ty -= carry * tiles_y;
        c.y0 = ty * TH;
        c.b += st_b + carry;
    };

    f32x4 acc[NCB][R][2];
    constexpr bool FLAT = C::FLAT;
    constexpr int FI = C::FI;
    u32x4 mreg[(MASK && X4) ? (FLAT ? FI : CC) : 1];      // ReLU-mask quads of the chunk in flight (this lane's part of the tile)
    unsigned goff_f[FLAT ? FI : 1];         // FLAT: per-item offsets (pixel + channel * plane) of this lane's DMA items
    float bias_r[NCB];           // bias of the tile whose first chunk was queued last (0 without a bias / under ksplit)
    using BC = BitsCfg<NCB, R>;
    unsigned bits_nxt[EPI == 5 ? BC::WPL : 1], bits_cur[EPI == 5 ? BC::WPL : 1];      // mask words of the tile queued last / being computed
    unsigned goff[XI];
    auto set_goff = [&](const TileCoord& t) {
        if constexpr (FLAT) {
#pragma unroll
            for (int k = 0; k < FI; ++k) {
                const int qi = tid + k * 256;
                const int c = qi / C::XNP, l = qi - c * C::XNP;
                const int ty = l / (TCOLS / 4), q = l - ty * (TCOLS / 4);
                const int gy = t.y0 + ty - PAD, gx = t.x0 - 4 + 4 * q;
                const bool ok = l < C::XN && gy >= 0 && gy < H && gx >= 0 && gx < W;
                goff_f[k] = ok ? (unsigned)(gy * W + gx) * 4u + (unsigned)c * plane_bytes : 0x80000000u;
            }
            return;
        }
#pragma unroll
        for (int k = 0; k < XI; ++k) {
            const int i = tid + k * 256;
            if constexpr (X4) {
                const int ty = i / (TCOLS / 4), q = i - ty * (TCOLS / 4);
                const int gy = t.y0 + ty - PAD, gx = t.x0 - 4 + 4 * q;
                const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
                goff[k] = ok ? (unsigned)(gy * W + gx) * 4u : 0x80000000u;
            } else {
                const int ty = i / TCOLS, tx = i - ty * TCOLS;
                const int gy = t.y0 + ty - PAD, gx = t.x0 + tx - PAD;
                const bool ok = i < PLANE && gy >= 0 && gy < H && gx >= 0 && gx < W;
                goff[k] = ok ? (unsigned)(gy * W + gx) * 4u : 0x80000000u;
            }
        }
    };
    // per-lane byte offsets of the filter quads inside a chunk's filter slice (the same for every chunk)
    constexpr int ROW4 = CB / 4;
    constexpr int WN = CC * KK * ROW4;                 // filter float4 per chunk
    constexpr int WI = (WN + 255) / 256;
    unsigned woff[WI];
#pragma unroll
    for (int k = 0; k < WI; ++k) {
        const int i = tid + k * 256;
        const int row = i / ROW4, j4 = i - row * ROW4;
        woff[k] = i < WN ? (unsigned)row * wrow_bytes + (unsigned)j4 * 16u : 0x80000000u;
    }
    const unsigned oob = 0x80000000u + (unsigned)(lane & 0);      // a VGPR holding the out-of-range marker

    // valid channels of chunk j of the (virtual) concatenation; scalar code only
    auto chunk_cnt = [&](int j) {
        const conv_kargs_t kb = conv_kargs();
        int s = 0, cs = kb->src[0].c;
        while (s + 1 < nsrc && j >= (cs + CC - 1) / CC) {
            j -= (cs + CC - 1) / CC;
            ++s;
            cs = kb->src[s].c;
        }
        return min(CC, cs - j * CC);
    };
    // issue the DMA of chunk j of tile t into buffer `buf` (and, with the tile's first chunk, the load of its bias)
    auto dma_chunk = [&](const TileCoord& t, int j, int buf, bool first, int tile_idx) {
        const conv_kargs_t kb = conv_kargs();
        int s = 0, cs = kb->src[0].c, start = 0;
        while (s + 1 < nsrc && j >= (cs + CC - 1) / CC) {
            j -= (cs + CC - 1) / CC;
            start += cs;
            ++s;
            cs = kb->src[s].c;
        }
        const int cnt = min(CC, cs - j * CC), cglob = start + j * CC;
        const int bmod = kb->src[s].bmod;
        const float* base = kb->src[s].p + (long long)(bmod > 0 ? t.b % bmod : t.b) * kb->src[s].bs + (long long)(j * CC) * HW;
        const __amdgpu_buffer_rsrc_t rx = sgpr_rsrc(base, (unsigned)cnt * plane_bytes);
        const unsigned xdst = lds0 + (unsigned)(buf * C::BUF_FLOATS) * 4u;
        // channels past the source's end (cnt < CC) are zero-filled through the marker offset
        if constexpr (FLAT) {
            // (channels past the source's end lie outside the descriptor: the range check zero-fills them)
#pragma unroll
            for (int k = 0; k < FI; ++k)
                if (tid + k * 256 < C::NITEM) dma16s(rx, xdst + (unsigned)(k * 256 + wave * 64) * 16u, goff_f[k], 0u);
        } else if constexpr (X4) {
            if (tid < C::XN) {
#pragma unroll
                for (int c = 0; c < CC; ++c) {
                    if (c < cnt) dma16s(rx, xdst + (unsigned)(c * CHS + wave * 256) * 4u, goff[0], (unsigned)c * plane_bytes);
                    else dma16s(rx, xdst + (unsigned)(c * CHS + wave * 256) * 4u, oob, 0u);
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < CC; ++c)
#pragma unroll
                for (int k = 0; k < XI; ++k) {
                    if (c < cnt) dma4s(rx, xdst + (unsigned)(c * CHS + k * 256 + wave * 64) * 4u, goff[k], (unsigned)c * plane_bytes);
                    else dma4s(rx, xdst + (unsigned)(c * CHS + k * 256 + wave * 64) * 4u, oob, 0u);
                }
        }
        if (MASK) {
            const __amdgpu_buffer_rsrc_t rm =
                sgpr_rsrc(kb->mask + (long long)t.b * kb->mask_bs + (long long)cglob * HW, (unsigned)cnt * plane_bytes);
            if constexpr (FLAT) {
#pragma unroll
                for (int k = 0; k < FI; ++k)
                    if (tid + k * 256 < C::NITEM) mreg[k] = __builtin_amdgcn_raw_buffer_load_b128(rm, goff_f[k], 0u, 0);
            } else if constexpr (X4) {
                // the mask quads go to registers (not through LDS): no second tile image -> 32 KB instead of
                // 55 KB of LDS per workgroup, and no LDS traffic for them; consumed by mask_in_place after the
                // wait that precedes the next barrier
                if (tid < C::XN) {
#pragma unroll
                    for (int c = 0; c < CC; ++c)
                        if (c < cnt) mreg[c] = __builtin_amdgcn_raw_buffer_load_b128(rm, goff[0], (unsigned)c * plane_bytes, 0);
                }
            } else {
                const unsigned mdst = xdst + (unsigned)C::XS_FLOATS * 4u;
#pragma unroll
                for (int c = 0; c < CC; ++c)
#pragma unroll
                    for (int k = 0; k < XI; ++k) {
                        if (c < cnt) dma4s(rm, mdst + (unsigned)(c * CHS + k * 256 + wave * 64) * 4u, goff[k], (unsigned)c * plane_bytes);
                        else dma4s(rm, mdst + (unsigned)(c * CHS + k * 256 + wave * 64) * 4u, oob, 0u);
                    }
            }
        }
        // filter rows cglob .. cglob+CC-1, columns cg*CB .. +CB-1: 16 bytes per lane
        const float* wsrc = kb->wp + (long long)cglob * KK * (long long)(wrow_bytes / 4u) + t.cg * CB;
        const __amdgpu_buffer_rsrc_t rw = sgpr_rsrc(wsrc, (unsigned)(CC * KK) * wrow_bytes);
        const unsigned wdst = xdst + (unsigned)(C::XS_FLOATS * ((MASK && !X4) ? 2 : 1)) * 4u;
#pragma unroll
        for (int k = 0; k < WI; ++k)
            if (tid + k * 256 < WN) dma16s(rw, wdst + (unsigned)(k * 256 + wave * 64) * 16u, woff[k], 0u);
        if (first) {
            // range check: channels >= cout read 0; no bias (dgrad) or a split channel loop: a zero-size buffer
            const float* bp = ksplit > 1 ? nullptr : kb->bias;
            const __amdgpu_buffer_rsrc_t rb = sgpr_rsrc(bp, (unsigned)kb->cout * 4u);
#pragma unroll
            for (int i = 0; i < NCB; ++i)
                bias_r[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, (unsigned)(i * 16 + r16) * 4u, (unsigned)(t.cg * CB) * 4u, 0));
            if constexpr (EPI == 5) {
                const __amdgpu_buffer_rsrc_t rq = sgpr_rsrc(kb->bits_in, 0x7fffffffu);
#pragma unroll
                for (int w = 0; w < BC::WPL; ++w)
                    bits_nxt[w] = __builtin_amdgcn_raw_buffer_load_b32(rq, (unsigned)(tid * BC::WPL + w) * 4u, (unsigned)tile_idx * (unsigned)(256 * BC::WPL * 4), 0);
            }
        }
    };

    auto mfma_chunk = [&](int cnt, int buf) {
        const int ngroups = (cnt + 3) / 4;
        // pixel lane r16 of a 16-pixel group: row r16 / TW, column r16 % TW of the (folded) row unit
        const float* xb = xs_of(buf) + kq * CHS + (wave * R * FOLD + r16 / TW) * TCOLS + (r16 % TW) + C::XOFF;
        const float* mb = xb;
        const float* wb = ws_of(buf) + kq * KK * CB + r16;
        auto rd = [&](const float* xp, const float*, int off) { return xp[off]; };      // (a dgrad's tile was masked in place)
        float a_cur[R][2], b_cur[NCB], a_nxt[R][2], b_nxt[NCB];
#pragma unroll
        for (int i = 0; i < NCB; ++i) b_cur[i] = wb[i * 16];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            a_cur[r][0] = rd(xb, mb, r * FOLD * TCOLS);
            a_cur[r][1] = rd(xb, mb, r * FOLD * TCOLS + C::GOFF);
        }
#pragma unroll 1
        for (int g = 0; g < ngroups; ++g) {
            const float* xp = xb + 4 * g * CHS;
            const float* mp = mb + 4 * g * CHS;
            const float* wq = wb + 4 * g * KK * CB;
#pragma unroll
            for (int t = 0; t < KK; ++t) {
                const int tn = (t + 1) % KK;
                const float* xn = t + 1 < KK ? xp : xp + 4 * CHS;
                const float* mn = t + 1 < KK ? mp : mp + 4 * CHS;
                const float* wn = t + 1 < KK ? wq : wq + 4 * KK * CB;
                const int kyn = tn / KS, kxn = tn % KS;
                if (t + 1 < KK || g + 1 < ngroups) {
#pragma unroll
                    for (int i = 0; i < NCB; ++i) b_nxt[i] = wn[tn * CB + i * 16];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        a_nxt[r][0] = rd(xn, mn, (r * FOLD + kyn) * TCOLS + kxn);
                        a_nxt[r][1] = rd(xn, mn, (r * FOLD + kyn) * TCOLS + kxn + C::GOFF);
                    }
                }
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int i = 0; i < NCB; ++i) {
                        acc[i][r][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[r][0], b_cur[i], acc[i][r][0], 0, 0, 0);
                        acc[i][r][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[r][1], b_cur[i], acc[i][r][1], 0, 0, 0);
                    }
#pragma unroll
                for (int i = 0; i < NCB; ++i) b_cur[i] = b_nxt[i];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    a_cur[r][0] = a_nxt[r][0];
                    a_cur[r][1] = a_nxt[r][1];
                }
            }
        }
    };

    // ReLU mask of a dgrad: dy is zeroed where the layer's activation was not positive.  Each lane rewrites, in
    // LDS, exactly the elements its own DMA instructions delivered (complete after this wave's vmcnt(0)), so no
    // extra barrier is needed, and the MFMA loop reads plain operands: 32 vector-ALU instructions per chunk and
    // lane instead of 144 selects inside the MFMA stream.
    auto mask_in_place = [&](int buf, int cnt) {
        float* xs = xs_of(buf);
        if constexpr (FLAT) {
#pragma unroll
            for (int k = 0; k < FI; ++k) {
                if (tid + k * 256 < C::NITEM) {      // (quads of channels past the source's end: x and mask both read 0)
                    f32x4* xp = reinterpret_cast<f32x4*>(xs) + (tid + k * 256);
                    const f32x4 m = __builtin_bit_cast(f32x4, mreg[k]);
                    f32x4 v = *xp;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.f ? v[e] : 0.f;
                    *xp = v;
                }
            }
        } else if constexpr (X4) {
            if (tid < C::XN) {
#pragma unroll
                for (int c = 0; c < CC; ++c) {
                    if (c < cnt) {          // (channels past the source's end are zeros already)
                        f32x4* xp = reinterpret_cast<f32x4*>(xs + c * CHS) + tid;
                        const f32x4 m = __builtin_bit_cast(f32x4, mreg[c]);
                        f32x4 v = *xp;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.f ? v[e] : 0.f;
                        *xp = v;
                    }
                }
            }
        } else {
            const float* ms = ms_of(buf);
#pragma unroll
            for (int c = 0; c < CC; ++c)
#pragma unroll
                for (int k = 0; k < XI; ++k) {
                    const int i = c * CHS + k * 256 + tid;
                    xs[i] = ms[i] > 0.f ? xs[i] : 0.f;
                }
        }
    };

    // Epilogue.  D = pixels x cout: lane (r16, kq) owns output channel cg*CB + 16 i + r16 and, in acc[i][r][g],
    // the four consecutive pixels x0 + 16 g + 4 kq .. +3 of row y0 + wave*R + r -> one 16-byte buffer store each.
    // The bias is already in the accumulators.  Per destination the descriptor covers exactly its channels of
    // image b, the per-lane offset carries (channel - first channel of the destination) and the column (lanes of
    // another destination, of channels >= cout, or of columns >= W fall outside the descriptor and are dropped by
    // the range check), the row goes into the scalar offset: ~10 vector-ALU instructions per destination.
    auto epilogue = [&](const TileCoord& t, int tile_idx) {
        const conv_kargs_t ke = conv_kargs();
        unsigned lo[NCB][2];       // ((16 i + r16) * HW + row-in-unit * W + x) * 4 for the two pixel groups, marker when x >= W
#pragma unroll
        for (int i = 0; i < NCB; ++i)
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const int q0 = 16 * g + 4 * kq;                     // first of this lane's 4 pixels in the 32-pixel row unit
                const int gx = t.x0 + q0 % TW;
                lo[i][g] = gx < W ? (unsigned)((i * 16 + r16) * HW + (q0 / TW) * W + gx) * 4u : 0x80000000u;
            }
        const int ybase = t.y0 + wave * R * FOLD;    // (H % FOLD == 0: a row unit lies wholly inside or outside the image)
        const int c_lo = t.cg * CB;        // first output channel of this tile
        if constexpr (EPI == 1) {
            // + the batch-shared part of the convolution (see ConvArgs::addend): the tile of image b % bmod, read with the
            // addressing of the stores below (lanes past the image / past cout fall outside the descriptor and add 0)
            const int abm = ke->addend_bmod;
            const float* ap = ke->addend + (long long)(abm > 0 ? t.b % abm : t.b) * ke->addend_bs;
            const __amdgpu_buffer_rsrc_t ra = sgpr_rsrc(ap, (unsigned)ke->cout * plane_bytes);
            const unsigned ub = (unsigned)(c_lo * HW + ybase * W) * 4u;
#ifdef YNET_ADD_PREFETCH
            // (experiment, round 4: ALL addend quads in flight at once -- one round trip instead of NCB * 2 batches of R, but NCB * R * 8 more
            // registers: 176 VGPRs for <2,4,4> = two resident workgroups per CU instead of four; measured on C5: see DESIGN.md section 8, 4b)
            f32x4 ad[NCB][R][2];
#pragma unroll
            for (int i = 0; i < NCB; ++i)
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const unsigned vo = lo[i][g] + ub;
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        ad[i][r][g] = (ybase + r * FOLD < H) ? __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, vo, (unsigned)(r * FOLD * W) * 4u, 0))
                                                             : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int i = 0; i < NCB; ++i)
#pragma unroll
                for (int g = 0; g < 2; ++g)
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[i][r][g] += ad[i][r][g];
#else
#pragma unroll
            for (int i = 0; i < NCB; ++i)
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const unsigned vo = lo[i][g] + ub;
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (ybase + r * FOLD < H)
                            acc[i][r][g] += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, vo, (unsigned)(r * FOLD * W) * 4u, 0));
                }
#endif
        }
        if (ke->relu && ksplit == 1) {
#pragma unroll
            for (int i = 0; i < NCB; ++i)
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int g = 0; g < 2; ++g)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[i][r][g][e] = acc[i][r][g][e] < 0.f ? 0.f : acc[i][r][g][e];
        }
        if constexpr (EPI == 2) if (ksplit == 1) {
            // ReLU backward on the OUTPUT (ConvArgs::emask): the activation values of the tile, read with the addressing of the
            // stores below (a separate instantiation: the values in flight cost up to 40 registers = one of the four workgroups
            // resident per CU, which the launches without this mask keep)
            const __amdgpu_buffer_rsrc_t re = sgpr_rsrc(ke->emask + (long long)t.b * ke->emask_bs, (unsigned)ke->cout * plane_bytes);
            const unsigned ub = (unsigned)(c_lo * HW + ybase * W) * 4u;
#pragma unroll
            for (int i = 0; i < NCB; ++i)
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const unsigned vo = lo[i][g] + ub;
                    f32x4 em[R];
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        em[r] = (ybase + r * FOLD < H) ? __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(re, vo, (unsigned)(r * FOLD * W) * 4u, 0))
                                                       : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int r = 0; r < R; ++r)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[i][r][g][e] = em[r][e] > 0.f ? acc[i][r][g][e] : 0.f;
                }
        }
        if constexpr (EPI == 4) {
            // the 1-bit form of this (post-ReLU) tile's activation mask: bit = value > 0 (NaN and -0: 0, as the float comparison of the
            // consumers), two vector instructions per element (compare into vcc, add-with-carry = shift the bit in)
            unsigned wv[BC::WPL];
#pragma unroll
            for (int w = 0; w < BC::WPL; ++w) wv[w] = 0u;
#pragma unroll
            for (int i = 0; i < NCB; ++i)
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int g = 0; g < 2; ++g)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int j = ((i * R + r) * 2 + g) * 4 + e;
                            asm volatile("v_cmp_gt_f32 vcc, %1, 0\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(wv[j >> 5]) : "v"(acc[i][r][g][e]) : "vcc");
                        }
            const __amdgpu_buffer_rsrc_t rq = sgpr_rsrc(ke->bits_out, 0x7fffffffu);
#pragma unroll
            for (int w = 0; w < BC::WPL; ++w)
                __builtin_amdgcn_raw_buffer_store_b32(wv[w], rq, (unsigned)(tid * BC::WPL + w) * 4u, (unsigned)tile_idx * (unsigned)(256 * BC::WPL * 4), 0);
        }
        if constexpr (EPI == 5) {
            // ReLU backward on the OUTPUT from the bit mask the forward convolution of the layer below wrote for this very tile
#pragma unroll
            for (int i = 0; i < NCB; ++i)
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int g = 0; g < 2; ++g)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int j = ((i * R + r) * 2 + g) * 4 + e;
                            const int pos = BC::count(j >> 5) - 1 - (j & 31);
                            const int m = __builtin_amdgcn_sbfe((int)bits_cur[j >> 5], pos, 1);       // 0 or -1
                            const float v = acc[i][r][g][e];       // (a scalar copy first: __builtin_bit_cast of the vector ELEMENT reads element 0)
                            acc[i][r][g][e] = __builtin_bit_cast(float, __builtin_bit_cast(int, v) & m);
                        }
        }
        if constexpr (EPI == 3) {
            // MaxPool2d(2, 2) of the tile: a lane holds 4 consecutive pixels of R rows per channel -- two pooled pixels per row pair,
            // one 8-byte store (the same first-maximum / NaN rule as maxpool2_fwd_kernel).  R and the tile origin are even.
            static_assert(R % 2 == 0 && FOLD == 1, "pooled epilogue: row pairs inside a wave's rows");
            typedef float f32x2e __attribute__((ext_vector_type(2)));
            typedef unsigned u32x2e __attribute__((ext_vector_type(2)));
            float* pp = ke->pool;
            const int Wo = W >> 1, HWo = (H >> 1) * Wo;
            const __amdgpu_buffer_rsrc_t rp = sgpr_rsrc(pp + (long long)t.b * ke->pool_bs, (unsigned)ke->cout * (unsigned)HWo * 4u);
#pragma unroll
            for (int i = 0; i < NCB; ++i)
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const int q0 = 16 * g + 4 * kq, gx = t.x0 + q0;
                    const unsigned vo = gx < W ? (unsigned)((c_lo + i * 16 + r16) * HWo + (gx >> 1)) * 4u : 0x80000000u;
#pragma unroll
                    for (int r = 0; r < R; r += 2) {
                        if (ybase + r < H) {
                            const f32x4 a = acc[i][r][g], b = acc[i][r + 1][g];
                            f32x2e o;
#pragma unroll
                            for (int h = 0; h < 2; ++h) {
                                // max of the 2 x 2 window, NaN if any of the four is (maxpool2_fwd_kernel's rule: its chain of
                                // `v > m || v != v` selects is 12 vector instructions per pooled pixel; this form is 5 -- v_max3 + v_max
                                // ignore NaNs, two unordered compares find them)
                                const float a0 = a[2 * h], a1 = a[2 * h + 1], b0 = b[2 * h], b1 = b[2 * h + 1];
                                float m;
                                asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(a0), "v"(a1), "v"(b0));
                                asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(m), "v"(b1));
                                const bool any_nan = __builtin_isunordered(a0, a1) | __builtin_isunordered(b0, b1);
                                o[h] = any_nan ? __builtin_nanf("") : m;
                            }
                            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2e, o), rp, vo, (unsigned)(((ybase + r) >> 1) * Wo) * 4u, 0);
                        }
                    }
                }
        }
        auto store_all = [&](__amdgpu_buffer_rsrc_t rd, unsigned ubase) {
            // ubase = ((c_lo - first channel of the destination) * HW + ybase * W) * 4, modulo 2^32
#pragma unroll
            for (int i = 0; i < NCB; ++i)
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const unsigned vo = lo[i][g] + ubase;
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (ybase + r * FOLD < H)
                            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[i][r][g]), rd, vo, (unsigned)(r * FOLD * W) * 4u, 0);
                }
        };
        if (ksplit > 1) {
            const int cout = ke->cout;
            float* pp = ke->partial + ((long long)t.ks * ke->B + t.b) * cout * (long long)HW;
            store_all(sgpr_rsrc(pp, (unsigned)cout * plane_bytes), (unsigned)(c_lo * HW + ybase * W) * 4u);
        } else {
            const int ndst = ke->ndst;
            int d_lo = 0;
#pragma unroll 1
            for (int d = 0; d < ndst; ++d) {
                const int dc = ke->dst[d].c;
                float* dp = ke->dst[d].p;
                // destinations this tile's channels do not touch (and unwanted ones) are skipped outright
                if (dp != nullptr && d_lo < c_lo + CB && d_lo + dc > c_lo)
                    store_all(sgpr_rsrc(dp + (long long)t.b * ke->dst[d].bs, (unsigned)dc * plane_bytes),
                              (unsigned)((c_lo - d_lo) * HW + ybase * W) * 4u);
                d_lo += dc;
            }
        }
    };

    // ---- load cursor one chunk ahead of the compute cursor; buffers alternate per flattened chunk
    int lt_idx = tile_first, lch = 0;
    if (lt_idx >= ntiles) return;
    TileCoord lt = decode(lt_idx);
    set_goff(lt);
    int lcnt = item_chunks(lt);
    auto advance_load = [&]() {
        if (++lch == lcnt) {
            lch = 0;
            lt_idx += gstride;
            if (lt_idx < ntiles) {
                advance_tile(lt);
                lcnt = item_chunks(lt);
                set_goff(lt);
            }
        }
    };
    dma_chunk(lt, lt.ks * cps, 0, true, lt_idx);
    advance_load();

    int ct_idx = tile_first, cch = 0, buf = 0, pt_idx = tile_first;
    TileCoord ct = decode(ct_idx), pt = ct;
    int ccnt = item_chunks(ct);
    bool pending = false;
    for (;;) {
        const bool have = ct_idx < ntiles;
        // this wave's DMAs of the chunk about to be consumed have landed; after the barrier every wave's
        // have, and every wave is done reading the other buffer
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (MASK && have) mask_in_place(buf, chunk_cnt(ct.ks * cps + cch));
        __syncthreads();
        if (pending) {
            epilogue(pt, pt_idx);
            pending = false;
        }
        if (!have) break;
        if (cch == 0) {
            // (the bias load was queued with this tile's first DMA, a chunk ago: consume it here so that hipcc
            // places its wait before the next DMAs are queued, where the counter is already 0)
#pragma unroll
            for (int i = 0; i < NCB; ++i) asm volatile("" : "+v"(bias_r[i]));
            if constexpr (EPI == 5) {
#pragma unroll
                for (int w = 0; w < BC::WPL; ++w) {
                    asm volatile("" : "+v"(bits_nxt[w]));
                    bits_cur[w] = bits_nxt[w];
                }
            }
#pragma unroll
            for (int i = 0; i < NCB; ++i)
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[i][r][0][q] = acc[i][r][1][q] = bias_r[i];
        }
        if (lt_idx < ntiles) {
            dma_chunk(lt, lt.ks * cps + lch, buf ^ 1, lch == 0, lt_idx);
            advance_load();
        }
        mfma_chunk(chunk_cnt(ct.ks * cps + cch), buf);
        buf ^= 1;
        if (++cch == ccnt) {
            cch = 0;
            pending = true;
            pt = ct;
            pt_idx = ct_idx;
            ct_idx += gstride;
            if (ct_idx < ntiles) {
                advance_tile(ct);
                ccnt = item_chunks(ct);
            }
        }
    }
}

template <int NCB, int R, int CC, bool MASK, bool X4, int FOLD>
__global__ __launch_bounds__(256, 2) void conv_dma_kernel(const ConvArgs) {
    conv_dma_body<NCB, R, CC, MASK, X4, FOLD, 0>();
}

// the same with the batch-shared additive term (ConvArgs::addend) in the epilogue
template <int NCB, int R, int CC, bool MASK, bool X4, int FOLD>
__global__ __launch_bounds__(256, 2) void conv_dma_add_kernel(const ConvArgs) {
    conv_dma_body<NCB, R, CC, MASK, X4, FOLD, 1>();
}

// the same with the 2 x 2 max-pooled copy of the output as a second destination (ConvArgs::pool)
template <int NCB, int R, int CC, bool MASK, bool X4, int FOLD>
__global__ __launch_bounds__(256, 2) void conv_dma_pool_kernel(const ConvArgs) {
    conv_dma_body<NCB, R, CC, MASK, X4, FOLD, 3>();
}

// the same with the ReLU backward of the layer below applied to the output (ConvArgs::emask)
template <int NCB, int R, int CC, bool MASK, bool X4, int FOLD>
__global__ __launch_bounds__(256, 2) void conv_dma_emask_kernel(const ConvArgs) {
    conv_dma_body<NCB, R, CC, MASK, X4, FOLD, 2>();
}

// the same with the 1-bit activation mask of the post-ReLU output as a second product (ConvArgs::bits_out)
template <int NCB, int R, int CC, bool MASK, bool X4, int FOLD>
__global__ __launch_bounds__(256, 2) void conv_dma_bits_kernel(const ConvArgs) {
    conv_dma_body<NCB, R, CC, MASK, X4, FOLD, 4>();
}

// the same with the ReLU backward of the layer below applied to the output from its 1-bit mask (ConvArgs::bits_in)
template <int NCB, int R, int CC, bool MASK, bool X4, int FOLD>
__global__ __launch_bounds__(256, 2) void conv_dma_emaskb_kernel(const ConvArgs) {
    conv_dma_body<NCB, R, CC, MASK, X4, FOLD, 5>();
}

// ================================================================================================
// Host side.  make_direct_plan decides which kernel a call takes (pure host arithmetic: no HIP call, no allocation);
// conv_dispatch_kernels maps the plan's fields to a template instantiation and launches it; the shape queries of the C ABI
// (ynet_conv2d_plan, ynet_conv2d_*_supported, ynet_conv2d_relu_bits_words) read the same plan.
// ================================================================================================

// The development switches of this dispatcher (A/B measurements only), read from the environment once per process.
struct ConvGates {
    int dma;            // YNET_CONV_DMA: the LDS-DMA generation (0: every call takes the register-staged tiles)
    int fold;           // YNET_CONV_FOLD: folded row units for maps no wider than 16 / 8 pixels
    // YNET_CONV_NARROW: work items a launch is narrowed towards (0: off).  Measured on the captured C2 step (MI355X): target 0 / 512 /
    // 1024 / 2048 / 4096 work items -> 9.78 / 9.69 / 9.63 / 9.56 / 9.55 ms at B = 32 and 4.05 / 3.88 / 3.84 / 3.79 / 3.79 ms at the
    // reference scripts' batch of 10; the 16^2 .. 64^2 layers need less (or no) split of the channel loop with it.
    int narrow;
    int rows;           // YNET_CONV_R: 1 / 2 / 4 forces the rows per wave
    int r4_min;         // YNET_CONV_R4_MIN: four rows per wave from this many four-row units
    // YNET_CONV_R2_MIN: two rows per wave from this many two-row units (round 4: 512 -> 64.  At the reference scripts' batch of 10 the
    // 32^2 / 64^2 layers fell below 512 two-row units and took the register-staged one-row kernel at 17-25 TFLOP/s; the two-row LDS-DMA
    // tile runs them at 22-37: captured step 3.49 -> 3.44 ms at B 10, 8.93 -> 8.90 at B 32; 32 and 128 measure the same as 64)
    int r2_min;
    int stream1;        // YNET_CONV_1X1_STREAM: the streaming kernel for the 1x1 predictors
    int no_ksplit;      // YNET_CONV_NO_KSPLIT (set, to any value): never split the channel loop
    int ksplit_items;   // YNET_KSPLIT_ITEMS: launches with fewer work items than this are split ...
    int ksplit_target;  // YNET_KSPLIT_TARGET: ... towards this many
    int relu_bits;      // YNET_RELU_BITS: the 1-bit activation masks (0: ynet_conv2d_relu_bits_words serves no shape)
    int debug;          // YNET_CONV_DEBUG -> ConvArgs::debug
};

static const ConvGates& conv_gates() {
    static const ConvGates g = {ynet_env_int("YNET_CONV_DMA", 1),        ynet_env_int("YNET_CONV_FOLD", 1),
                                ynet_env_int("YNET_CONV_NARROW", 2048),  ynet_env_int("YNET_CONV_R", 0),
                                ynet_env_int("YNET_CONV_R4_MIN", 1024),  ynet_env_int("YNET_CONV_R2_MIN", 64),
                                ynet_env_int("YNET_CONV_1X1_STREAM", 1), getenv("YNET_CONV_NO_KSPLIT") ? 1 : 0,
                                ynet_env_int("YNET_KSPLIT_ITEMS", 256),  ynet_env_int("YNET_KSPLIT_TARGET", 512),
                                ynet_env_int("YNET_RELU_BITS", 1),       ynet_env_int("YNET_CONV_DEBUG", 0)};
    return g;
}

// Split of the input-channel loop over workgroups for launches with fewer work items than CUs.
static int conv_ksplit(long long items, int nchunks) {
    const ConvGates& g = conv_gates();
    if (g.no_ksplit || items >= g.ksplit_items || nchunks < 4) return 1;
    long long k = (g.ksplit_target + items - 1) / items;
    if (k > nchunks / 2) k = nchunks / 2;
    if (k > 8) k = 8;
    return k < 1 ? 1 : (int)k;
}

// y = [relu](sum_ks partial[ks] + bias), scattered to the (possibly split) destination
struct SplitReduceArgs {
    const float* partial;
    const float* bias;
    YDst dst[YNET_MAX_SRC];
    int ndst, ksplit, B, cout, HW, relu;
    const float* emask;     // ConvArgs::emask (one destination): out = emask > 0 ? sum : 0
    long long emask_bs;
};

__global__ __launch_bounds__(256) void conv_split_reduce_kernel(const SplitReduceArgs a) {
    const long long n4 = (long long)a.B * a.cout * (a.HW >> 2);
    const int hw4 = a.HW >> 2;
    const long long slab = (long long)a.B * a.cout * a.HW;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const int p4 = (int)(i % hw4);
        const int co = (int)((i / hw4) % a.cout);
        const int b = (int)(i / ((long long)hw4 * a.cout));
        f32x4 s = *reinterpret_cast<const f32x4*>(a.partial + i * 4);
        for (int k = 1; k < a.ksplit; ++k) s += *reinterpret_cast<const f32x4*>(a.partial + k * slab + i * 4);
        const float bv = a.bias ? a.bias[co] : 0.f;
        int rel = co, d = 0;
        while (d < a.ndst - 1 && rel >= a.dst[d].c) {
            rel -= a.dst[d].c;
            ++d;
        }
        float* dp = a.dst[d].p;
        if (dp == nullptr) continue;
        dp += (long long)b * a.dst[d].bs + (long long)rel * a.HW + p4 * 4;
        f32x4 m = f32x4{1.f, 1.f, 1.f, 1.f};
        if (a.emask) m = *reinterpret_cast<const f32x4*>(a.emask + (long long)b * a.emask_bs + (long long)co * a.HW + p4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float u = s[e] + bv;
            if (a.relu) u = u < 0.f ? 0.f : u;
            dp[e] = m[e] > 0.f ? u : 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The launch plan: everything the choice of a kernel consists of, from everything it depends on.
// ------------------------------------------------------------------------------------------------
enum { GEN_NONE = 0, GEN_REG = 1, GEN_DMA = 2, GEN_FOLD = 3, GEN_STREAM = 4 };      // 1 .. 4: the kind ynet_note_launch reports in bits 0 .. 3
enum { EPI_PLAIN = 0, EPI_ADD = 1, EPI_EMASK = 2, EPI_POOL = 3, EPI_BITS_OUT = 4, EPI_BITS_IN = 5 };      // conv_dma_body's EPI

struct DirectCall {
    int B, H, W, cout, K;       // cout: the channels left after the unwanted trailing destinations are dropped
    bool vec_load, vec_store;   // 16-byte loads / stores are legal (ConvArgs::vec_load / vec_store)
    bool mask, emask, pool, bits_out, bits_in, addend;      // the operand is present
    bool addend_ok;             // one destination, the additive term 16-byte aligned
    bool stream_ok;             // one source that does not repeat along the batch, one wanted destination (the 1x1 streaming kernel)
};

struct DirectPlan {
    int gen;            // GEN_*: register-staged / LDS-DMA / folded LDS-DMA / 1x1 stream; GEN_NONE: no kernel serves the call
    int nt16;           // 16-channel tiles the output channels are cut into (0: 32-channel blocks -- 1x1, 5x5)
    int tiles, cb;      // tiles (blocks) per workgroup = the kernels' NCB, and its output channels; stream: 16 tiles output channels per thread
    int rows, fold, cc; // rows per wave, folded row units (1: none), input channels per staged chunk
    bool may_split;     // the channel loop may be split over workgroups (where the caller gave a workspace)
    int epi;            // EPI_*: the epilogue extra the kernel itself applies (unfolded LDS-DMA tiles only; an output mask is applied
                        // elsewhere by the reduction of a split channel loop or a pass of its own, the other extras nowhere else)
};

// Rows per wave (R): 4 gives the most operand reuse; small feature maps (8^2 .. 64^2) take R = 2 or 1
// so that the launch still spreads over the 256 CUs (a workgroup's run time is its MFMA count).
static int pick_rows(const DirectCall& c, int cb) {
    const ConvGates& g = conv_gates();
    if (g.rows == 1 || g.rows == 2 || g.rows == 4) return g.rows;
    const long long per_img_x = ceil_div(c.W, 32), cg = ceil_div(c.cout, cb);
    for (int r = 4; r > 1; r >>= 1) {
        const long long nblk = per_img_x * ceil_div(c.H, 4 * r) * cg * c.B;
        if (nblk >= (r == 4 ? g.r4_min : g.r2_min)) return r;
    }
    return 1;
}

// Rows per wave of a launch with nt16 16-channel tiles per workgroup: pick_rows, but at most two with three or four tiles (four rows of
// them need more accumulators than a lane has registers: the register-staged kernel would spill, the LDS-DMA kernel has no such form).
static int dma_rows(const DirectCall& c, int nt16) {
    const int rows = pick_rows(c, 16 * nt16);
    return (nt16 >= 3 && rows == 4) ? 2 : rows;
}

// The 16-channel tiles of a 3x3 layer: Cout is padded to 16 / 32 / 48 / 64 per workgroup
static int m16_tiles(int cout) { return cout <= 16 ? 1 : (cout <= 32 ? 2 : (cout <= 48 ? 3 : 4)); }

static int conv_fold(int H, int W) {
    if (!conv_gates().fold) return 1;
    if (W <= 8 && (H & 3) == 0) return 4;
    if (W <= 16 && (H & 1) == 0) return 2;
    return 1;
}

// Small and mid-size maps: fewer output channels per workgroup -> more workgroups.  A 64 -> 64 layer on B x 32^2 pixels is 256
// row units: with all 64 output channels in one workgroup that is ONE workgroup per CU (one wave per SIMD, nothing to hide
// its staging latency behind); 16 channels per workgroup give four per CU and the same MFMA count in total (the input tile
// is then staged by four workgroups instead of one -- from L2).
static int narrow_tiles(const DirectCall& c, int nt16, int fold) {
    const int target = conv_gates().narrow;
    if (target <= 0 || nt16 <= 1) return nt16;
    const long long units = (long long)c.B * ceil_div(c.W, 32 / fold) * ceil_div(c.H, 4 * fold);      // one-row-per-wave tiles
    int n = nt16;
    while (n > 1 && units * ceil_div(nt16, n) < target) n = n > 2 ? 2 : 1;
    return n;
}

static DirectPlan make_direct_plan(const DirectCall& c) {
    const ConvGates& g = conv_gates();
    DirectPlan p{};
    p.fold = 1;
    p.epi = EPI_PLAIN;
    const int full = c.K == 3 ? m16_tiles(c.cout) : 0, fold = conv_fold(c.H, c.W);
    p.nt16 = c.addend ? full : narrow_tiles(c, full, fold);       // (the additive-term kernels exist for two and four tiles only)
    // 3x3 on 16-byte aligned operands: the LDS-DMA generation -- folded row units for maps no wider than 16 / 8 pixels, else tiles of
    // two or four rows per wave; a map too small for two-row units goes on to the register-staged one-row kernel.
    if (p.nt16 && g.dma && c.vec_load && c.vec_store) {
        const int rows = fold > 1 ? 1 : dma_rows(c, p.nt16);
        if (fold > 1 || rows >= 2) {
            p.gen = fold > 1 ? GEN_FOLD : GEN_DMA;
            p.tiles = p.nt16;
            p.cb = 16 * p.nt16;
            p.rows = rows;
            p.fold = fold;
            // CC = 4 input channels (one K-step of the 16x16x4 MFMA) per chunk: 34-60 KB of LDS for both buffers, so 3-4 workgroups stay
            // resident per CU (measured 5-10 % faster than CC = 8 with 2 resident workgroups).  The small tiles (folded maps, two rows of one
            // tile) take CC 8: a chunk of 4 channels is 18 .. 72 MFMAs per wave there -- 0.3 .. 1 us -- behind a DMA round trip of ~1.3 us
            // that the one-chunk-ahead pipeline cannot hide.  (Deeper chunks gain nothing: DESIGN.md section 4.17.)
            p.cc = (p.tiles <= 2 && (fold > 1 || (rows == 2 && p.tiles == 1))) ? 8 : 4;
            if (p.gen == GEN_DMA) {
                if (c.addend) p.epi = EPI_ADD;
                else if (c.bits_in) p.epi = EPI_BITS_IN;
                else if (c.bits_out && !c.mask) p.epi = EPI_BITS_OUT;
                else if (c.emask) p.epi = EPI_EMASK;
                else if (c.pool && !c.mask) p.epi = EPI_POOL;
            }
            p.may_split = p.epi == EPI_PLAIN || p.epi == EPI_EMASK;
        }
    }
    if (c.addend) {     // what evaluate()'s shared skip features need, nothing more; callers ask ynet_conv2d_add_supported first
        if (!(p.epi == EPI_ADD && (p.tiles == 2 || p.tiles == 4) && !c.mask && c.addend_ok)) p.gen = GEN_NONE;
        return p;
    }
    if (p.gen != GEN_NONE) return p;
    if (c.K == 1 && g.stream1 && c.stream_ok && !c.mask && c.cout <= 32 && c.vec_store && c.vec_load && ((long long)c.H * c.W) % 4 == 0) {
        p.gen = GEN_STREAM;
        p.tiles = c.cout <= 16 ? 1 : 2;
        p.cb = 16 * p.tiles;
        return p;
    }
    p.gen = (c.K == 1 || c.K == 3 || c.K == 5) ? GEN_REG : GEN_NONE;
    p.may_split = true;
    if (p.nt16) {
        p.tiles = p.nt16;
        p.cb = 16 * p.nt16;
        p.rows = dma_rows(c, p.nt16);
        p.cc = 8;
    } else {
        p.tiles = c.cout > 32 ? 2 : 1;
        p.cb = 32 * p.tiles;
        p.rows = c.K == 5 ? 4 : pick_rows(c, p.cb);
        p.cc = c.K == 1 ? 16 : 4;
    }
    return p;
}

// ------------------------------------------------------------------------------------------------
// Launches: plan fields -> template arguments.  Nothing below decides anything.
// ------------------------------------------------------------------------------------------------
// The tile launch both generations share: tile counts, the split of the channel loop under the workspace cap, the persistent grid and
// the reduction of a split.  `slots`: resident workgroups of this instantiation on this device (0: not asked yet).
static int conv_launch_tiles(ConvArgs& a, const DirectPlan& p, const void* kernel, int lds_bytes, int& slots, hipStream_t st) {
    a.tiles_x = ceil_div(a.W, 32 / p.fold);
    a.tiles_y = ceil_div(a.H, 4 * p.rows * p.fold);
    a.cgroups = ceil_div(a.cout, p.cb);
    long long nt = (long long)a.tiles_x * a.tiles_y * a.cgroups * a.B;
    {   // small maps: split the channel chunks over several workgroups (partials summed by a second kernel)
        int nchunks = 0;
        for (int i = 0; i < a.nsrc; ++i) nchunks += ceil_div(a.src[i].c, p.cc);
        a.ksplit = 1;
        if (a.partial != nullptr && p.may_split) a.ksplit = conv_ksplit(nt, nchunks);
        while (a.ksplit > 1 && (long long)a.ksplit * a.B * a.cout * a.H * a.W > a.partial_cap) --a.ksplit;
        a.cps = ceil_div(nchunks, a.ksplit);
        a.ksplit = ceil_div(nchunks, a.cps);          // no empty split
        nt *= a.ksplit;
    }
    YNET_REQUIRE(nt > 0 && nt < (1ll << 31), "conv2d: %lld tiles are out of range", nt);
    a.ntiles = (int)nt;
    a.debug = conv_gates().debug;
    if (slots == 0) {
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        int per_cu = 0, dev = 0, cus = 256;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, lds_bytes);
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (per_cu < 1) per_cu = 1;
        if (cus < 1) cus = 256;
        slots = per_cu * cus;
    }
    const long long nblk = nt < slots ? nt : slots;
    ynet_note_launch(0, p.gen | (p.rows << 4) | (a.ksplit << 8) | (a.vec_load << 12) | (a.vec_store << 13));
    void* kargs[] = {&a};
    (void)hipLaunchKernel(kernel, dim3((unsigned)nblk), dim3(256), kargs, lds_bytes, st);
    const bool reduce_emask = p.gen != GEN_REG;       // (the register-staged generation leaves the output mask to conv_emask_kernel)
    if (a.ksplit > 1) {
        SplitReduceArgs r{};
        r.partial = a.partial;
        r.bias = a.bias;
        for (int i = 0; i < a.ndst; ++i) r.dst[i] = a.dst[i];
        r.ndst = a.ndst;
        r.ksplit = a.ksplit;
        r.B = a.B;
        r.cout = a.cout;
        r.HW = a.H * a.W;
        r.relu = a.relu;
        if (reduce_emask) {
            r.emask = a.emask;
            r.emask_bs = a.emask_bs;
        }
        long long n4 = (long long)a.B * a.cout * (r.HW / 4);
        int grid = (int)((n4 + 255) / 256);
        if (grid > 2048) grid = 2048;
        hipLaunchKernelGGL(conv_split_reduce_kernel, dim3(grid), dim3(256), 0, st, r);
    }
    a.emask_done = p.epi == EPI_EMASK || (reduce_emask && a.ksplit > 1);      // (in the epilogue, or in the reduction of a split channel loop)
    return ynet_check_launch("conv2d");
}

template <int KS, int NCB, int R, int CC, bool M16>
static int launch_conv(ConvArgs& a, const DirectPlan& p, hipStream_t st) {
    static int slots_m[YNET_MAX_DEV] = {0}, slots_p[YNET_MAX_DEV] = {0};      // (per instantiation and per device)
    const int dev = ynet_device_slot();
    if (a.mask) return conv_launch_tiles(a, p, reinterpret_cast<const void*>(&conv_mfma_kernel<KS, NCB, R, CC, true, M16>), ConvCfg<KS, NCB, R, CC, M16>::LDS_BYTES, slots_m[dev], st);
    return conv_launch_tiles(a, p, reinterpret_cast<const void*>(&conv_mfma_kernel<KS, NCB, R, CC, false, M16>), ConvCfg<KS, NCB, R, CC, M16>::LDS_BYTES, slots_p[dev], st);
}

static int launch_plan_reg(ConvArgs& a, const DirectPlan& p, int K, hipStream_t st) {
#define REG_CASE(KS, NCB, R, CC, M16) \
    if (K == KS && p.tiles == NCB && p.rows == R && p.cc == CC) return launch_conv<KS, NCB, R, CC, M16>(a, p, st)
    REG_CASE(3, 1, 4, 8, true);  REG_CASE(3, 1, 2, 8, true);  REG_CASE(3, 1, 1, 8, true);
    REG_CASE(3, 2, 4, 8, true);  REG_CASE(3, 2, 2, 8, true);  REG_CASE(3, 2, 1, 8, true);
    REG_CASE(3, 3, 2, 8, true);  REG_CASE(3, 3, 1, 8, true);
    REG_CASE(3, 4, 2, 8, true);  REG_CASE(3, 4, 1, 8, true);
    REG_CASE(1, 1, 4, 16, false); REG_CASE(1, 1, 2, 16, false); REG_CASE(1, 1, 1, 16, false);
    REG_CASE(1, 2, 4, 16, false); REG_CASE(1, 2, 2, 16, false); REG_CASE(1, 2, 1, 16, false);
    REG_CASE(5, 1, 4, 4, false);  REG_CASE(5, 2, 4, 4, false);
#undef REG_CASE
    ynet_set_error("conv2d: no register-staged kernel for K=%d tiles=%d rows=%d", K, p.tiles, p.rows);
    return 1;
}

// Only the quad-DMA form (X4) is instantiated: the plan asks for vec_load.
template <int NCB, int R, int CC, bool MASK, int FOLD, int EPI>
static int launch_dma_m(ConvArgs& a, const DirectPlan& p, hipStream_t st) {
    const auto KERNEL = [] {       // (if constexpr: only the wanted instantiation is compiled)
        if constexpr (EPI == EPI_ADD) return &conv_dma_add_kernel<NCB, R, CC, MASK, true, FOLD>;
        else if constexpr (EPI == EPI_EMASK) return &conv_dma_emask_kernel<NCB, R, CC, MASK, true, FOLD>;
        else if constexpr (EPI == EPI_POOL) return &conv_dma_pool_kernel<NCB, R, CC, MASK, true, FOLD>;
        else if constexpr (EPI == EPI_BITS_OUT) return &conv_dma_bits_kernel<NCB, R, CC, MASK, true, FOLD>;
        else if constexpr (EPI == EPI_BITS_IN) return &conv_dma_emaskb_kernel<NCB, R, CC, MASK, true, FOLD>;
        else return &conv_dma_kernel<NCB, R, CC, MASK, true, FOLD>;
    }();
    static int slots_dev[YNET_MAX_DEV] = {0};          // resident workgroups on the device for this instantiation
    return conv_launch_tiles(a, p, reinterpret_cast<const void*>(KERNEL), DmaCfg<NCB, R, CC, MASK, true, FOLD>::LDS_BYTES, slots_dev[ynet_device_slot()], st);
}

// plan.epi and the input-side mask -> the kernel form.  The pooled copy and the written bit mask exist without an input-side mask only,
// the additive term for two and four tiles without one, and the folded tiles are plain.
template <int NCB, int R, int CC, int FOLD>
static int launch_dma(ConvArgs& a, const DirectPlan& p, hipStream_t st) {
    const bool m = a.mask != nullptr;
    if constexpr (FOLD == 1) {
        if (p.epi == EPI_BITS_IN) return m ? launch_dma_m<NCB, R, CC, true, 1, EPI_BITS_IN>(a, p, st) : launch_dma_m<NCB, R, CC, false, 1, EPI_BITS_IN>(a, p, st);
        if (p.epi == EPI_EMASK) return m ? launch_dma_m<NCB, R, CC, true, 1, EPI_EMASK>(a, p, st) : launch_dma_m<NCB, R, CC, false, 1, EPI_EMASK>(a, p, st);
        if (p.epi == EPI_BITS_OUT && !m) return launch_dma_m<NCB, R, CC, false, 1, EPI_BITS_OUT>(a, p, st);
        if (p.epi == EPI_POOL && !m) return launch_dma_m<NCB, R, CC, false, 1, EPI_POOL>(a, p, st);
        if constexpr (NCB == 2 || NCB == 4) {
            if (p.epi == EPI_ADD && !m) return launch_dma_m<NCB, R, CC, false, 1, EPI_ADD>(a, p, st);
        }
    }
    if (p.epi == EPI_PLAIN) return m ? launch_dma_m<NCB, R, CC, true, FOLD, EPI_PLAIN>(a, p, st) : launch_dma_m<NCB, R, CC, false, FOLD, EPI_PLAIN>(a, p, st);
    ynet_set_error("conv2d: no LDS-DMA kernel for tiles=%d rows=%d fold=%d with epilogue %d%s", NCB, R, FOLD, p.epi, m ? " and a mask" : "");
    return 1;
}

static int launch_plan_dma(ConvArgs& a, const DirectPlan& p, hipStream_t st) {
#define DMA_CASE(NCB, R, CC, FOLD) \
    if (p.tiles == NCB && p.rows == R && p.cc == CC && p.fold == FOLD) return launch_dma<NCB, R, CC, FOLD>(a, p, st)
    DMA_CASE(1, 4, 4, 1); DMA_CASE(1, 2, 8, 1);
    DMA_CASE(2, 4, 4, 1); DMA_CASE(2, 2, 4, 1);
    DMA_CASE(3, 2, 4, 1);
    DMA_CASE(4, 2, 4, 1);
    DMA_CASE(1, 1, 8, 2); DMA_CASE(1, 1, 8, 4);
    DMA_CASE(2, 1, 8, 2); DMA_CASE(2, 1, 8, 4);
    DMA_CASE(3, 1, 4, 2); DMA_CASE(3, 1, 4, 4);
    DMA_CASE(4, 1, 4, 2); DMA_CASE(4, 1, 4, 4);
#undef DMA_CASE
    ynet_set_error("conv2d: no LDS-DMA kernel for tiles=%d rows=%d chunk=%d fold=%d", p.tiles, p.rows, p.cc, p.fold);
    return 1;
}


// ================================================================================================
// 1x1 convolution with few output channels (the predictors: 32 -> pred_len, and their dgrad pred_len -> 32): 4.4-12
// FLOP per byte, HBM-bound.  One thread owns 4 consecutive pixels (16-byte loads / stores, a wave reads 1 KB
// contiguous per input channel) and all CT output channels; the filter row of each input channel arrives through
// scalar loads (uniform address) and feeds v_fmac from SGPRs.  fp32 FMA chain over the input channels in order.
// ================================================================================================
struct Conv1x1Args {
    const float* x;
    long long x_bs;
    const float* wp;        // packed [cin_pad][cout_pad]
    const float* bias;
    float* y;
    long long y_bs;
    int cin, cout, cout_pad, relu, B;
    long long hw4;          // H * W / 4
};

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) float* const_f32_ptr;      // uniform reads -> scalar loads

// PX pixels per thread (4: 16-byte accesses, CT <= 16; 2: 8-byte accesses, CT = 32 -> 64 accumulator registers)
template <int CT, int PX>
__global__ __launch_bounds__(256) void conv1x1_stream_kernel(const Conv1x1Args a) {
    typedef float vec_t __attribute__((ext_vector_type(PX)));
    const long long hwv = a.hw4 * (4 / PX);
    const long long total = (long long)a.B * hwv;
    const const_f32_ptr w = (const_f32_ptr)a.wp, bias = (const_f32_ptr)a.bias;
    for (long long q = blockIdx.x * 256ll + threadIdx.x; q < total; q += (long long)gridDim.x * 256) {
        const int b = (int)(q / hwv);
        const long long p = q - (long long)b * hwv;
        const vec_t* xp = reinterpret_cast<const vec_t*>(a.x + (long long)b * a.x_bs) + p;
        vec_t acc[CT];
#pragma unroll
        for (int co = 0; co < CT; ++co) {
            const float bv = (a.bias != nullptr && co < a.cout) ? bias[co] : 0.f;
#pragma unroll
            for (int e = 0; e < PX; ++e) acc[co][e] = bv;
        }
#pragma unroll 2
        for (int ci = 0; ci < a.cin; ++ci) {
            const vec_t v = xp[(long long)ci * hwv];
#pragma unroll
            for (int co = 0; co < CT; ++co) {
                const float wv = w[ci * a.cout_pad + co];
#pragma unroll
                for (int e = 0; e < PX; ++e) acc[co][e] = __builtin_fmaf(v[e], wv, acc[co][e]);
            }
        }
        vec_t* yp = reinterpret_cast<vec_t*>(a.y + (long long)b * a.y_bs) + p;
#pragma unroll
        for (int co = 0; co < CT; ++co) {
            if (co < a.cout) {
                vec_t o = acc[co];
                if (a.relu) {
#pragma unroll
                    for (int e = 0; e < PX; ++e) o[e] = o[e] < 0.f ? 0.f : o[e];
                }
                yp[(long long)co * hwv] = o;
            }
        }
    }
}

template <int CT, int PX>
static int launch_conv1x1_stream(const ConvArgs& a, hipStream_t st) {
    Conv1x1Args k{};
    k.x = a.src[0].p;
    k.x_bs = a.src[0].bs;
    k.wp = a.wp;
    k.bias = a.bias;
    k.y = a.dst[0].p;
    k.y_bs = a.dst[0].bs;
    k.cin = a.src[0].c;
    k.cout = a.cout;
    k.cout_pad = a.cout_pad;
    k.relu = a.relu;
    k.B = a.B;
    k.hw4 = (long long)a.H * a.W / 4;
    long long blocks = ((long long)a.B * k.hw4 * (4 / PX) + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    ynet_note_launch(0, 4 | (1 << 8) | (a.vec_load << 12) | (a.vec_store << 13));
    hipLaunchKernelGGL((conv1x1_stream_kernel<CT, PX>), dim3((unsigned)blocks), dim3(256), 0, st, k);
    return ynet_check_launch("conv2d(1x1)");
}

static int conv_dispatch_kernels(ConvArgs& a, const DirectPlan& p, int K, hipStream_t st) {
    switch (p.gen) {
        case GEN_DMA:
        case GEN_FOLD: return launch_plan_dma(a, p, st);
        case GEN_STREAM: return p.tiles == 1 ? launch_conv1x1_stream<16, 4>(a, st) : launch_conv1x1_stream<32, 2>(a, st);
        case GEN_REG: return launch_plan_reg(a, p, K, st);
    }
    if (a.addend != nullptr) ynet_set_error("conv2d_add: shape B=%d %dx%d cout=%d is not served by the additive-term kernels", a.B, a.H, a.W, a.cout);
    else ynet_set_error("conv2d: kernel size %d not supported (1, 3, 5)", K);
    return 1;
}

// dst = emask > 0 ? dst : 0 for the kernel families without the output-side mask in their epilogue (register-staged tiles,
// 1x1 streaming, 5x5): a separate pass, correct everywhere, fast nowhere -- the layers of the hot path take the LDS-DMA kernels.
__global__ __launch_bounds__(256) void conv_emask_kernel(float* __restrict__ dst, long long dst_bs, const float* __restrict__ emask,
                                                         long long emask_bs, long long per_image, long long total) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long b = i / per_image, o = i - b * per_image;
        if (!(emask[b * emask_bs + o] > 0.f)) dst[b * dst_bs + o] = 0.f;
    }
}

static int conv_dispatch(ConvArgs& a, int K, hipStream_t st) {
    DirectCall c{};
    c.B = a.B, c.H = a.H, c.W = a.W, c.cout = a.cout, c.K = K;
    c.vec_load = a.vec_load != 0;
    c.vec_store = a.vec_store != 0;
    c.mask = a.mask != nullptr;
    c.emask = a.emask != nullptr;
    c.pool = a.pool != nullptr;
    c.bits_out = a.bits_out != nullptr;
    c.bits_in = a.bits_in != nullptr;
    c.addend = a.addend != nullptr;
    c.addend_ok = a.ndst == 1 && (reinterpret_cast<uintptr_t>(a.addend) & 15) == 0 && (a.addend_bs & 3) == 0;
    c.stream_ok = a.nsrc == 1 && a.ndst == 1 && a.dst[0].p != nullptr && a.src[0].bmod == 0;
    const DirectPlan p = make_direct_plan(c);
    // The 1-bit masks and the pooled copy exist in the epilogues of the unfolded LDS-DMA tiles only: a plan without them is refused
    // before anything is launched.
    if ((c.bits_out || c.bits_in) && p.epi != EPI_BITS_OUT && p.epi != EPI_BITS_IN) {
        ynet_set_error("conv2d (bit mask): shape B=%d %dx%d cout=%d is not served by the bit-mask epilogues (ask ynet_conv2d_relu_bits_words)", a.B, a.H, a.W, a.cout);
        return 1;
    }
    if (c.pool && p.epi != EPI_POOL) {
        ynet_set_error("conv2d_pool: shape B=%d %dx%d cout=%d is not served by the pooling epilogue (ask ynet_conv2d_pool_supported)", a.B, a.H, a.W, a.cout);
        return 1;
    }
    a.emask_done = 0;
    const int rc = conv_dispatch_kernels(a, p, K, st);
    if (rc || a.emask == nullptr || a.emask_done) return rc;
    const long long per_image = (long long)a.cout * a.H * a.W, total = per_image * a.B;
    long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(conv_emask_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a.dst[0].p, a.dst[0].bs, a.emask, a.emask_bs, per_image, total);
    return ynet_check_launch("conv2d(output mask)");
}

// The largest CC used above: the packed filter is zero padded to a multiple of it along cin.
#define YNET_CIN_PAD 16
#define YNET_COUT_PAD 64

// ------------------------------------------------------------------------------------------------
// filter packing: checkpoint layout [Cout][Cin][K][K] -> [cin_pad][K*K][cout_pad] (zero padded)
//   mode 0 (forward): wp[ci][t][co] = w[co][ci][t]
//   mode 1 (dgrad):   wp[co][t][ci] = w[co][ci][K*K-1-t]   (roles of cin/cout swapped, taps flipped)
// ------------------------------------------------------------------------------------------------
__global__ void pack_weight_kernel(const float* __restrict__ w, float* __restrict__ wp, int cout, int cin,
                                   int KK, int mode, int rows /*K-dim channels*/, int cols /*M-dim channels*/,
                                   int rows_pad, int cols_pad) {
    const long long n = (long long)rows_pad * KK * cols_pad;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        const int m = (int)(i % cols_pad);
        const int t = (int)((i / cols_pad) % KK);
        const int k = (int)(i / ((long long)cols_pad * KK));
        float v = 0.f;
        if (k < rows && m < cols) {
            v = mode == 0 ? w[((long long)m * cin + k) * KK + t] : w[((long long)k * cin + m) * KK + (KK - 1 - t)];
        }
        wp[i] = v;
    }
}

extern "C" {

// The plan of a plain call of this shape on 16-byte aligned operands (W % 4 != 0: no operand is aligned), or of such a call with an
// additive term: what the shape queries below read.  It leaves the 1x1 streaming kernel out (its gates are on the operands), so a
// 1x1 shape names the tile kernel that an unaligned call takes.
static DirectPlan shape_plan(int B, int H, int W, int cout, int K, bool addend = false) {
    DirectCall c{};
    c.B = B, c.H = H, c.W = W, c.cout = cout, c.K = K;
    c.vec_load = c.vec_store = (W % 4) == 0;
    c.addend = c.addend_ok = addend;
    return make_direct_plan(c);
}

// The kernel instantiation the dispatcher picks for this problem, for naming it in profiles:
// returns rows | tiles << 8 | m16 << 16 | dma << 17 | x4 << 18 | log2(fold) << 19 | CC << 21
//   ->  conv_mfma_kernel<K, tiles, rows, CC, mask, m16> or, with dma, conv_dma_kernel<tiles, rows, CC, mask, x4, fold>
int ynet_conv2d_plan(int B, int H, int W, int cout, int K) {
    const DirectPlan p = shape_plan(B, H, W, cout, K);
    const int dma = (p.gen == GEN_DMA || p.gen == GEN_FOLD) ? 1 : 0;
    const int flog = p.fold == 4 ? 2 : (p.fold == 2 ? 1 : 0);
    return p.rows | (p.tiles << 8) | ((p.nt16 ? 1 : 0) << 16) | (dma << 17) | (dma << 18) | (flog << 19) | (p.cc << 21);
}

long long ynet_packed_weight_floats(int cout, int cin, int K, int mode) {
    const int rows = mode == 0 ? cin : cout, cols = mode == 0 ? cout : cin;
    const long long rp = (long long)ceil_div(rows, YNET_CIN_PAD) * YNET_CIN_PAD + YNET_CIN_PAD;   // + one chunk of slack rows
    const long long cp = (long long)ceil_div(cols, YNET_COUT_PAD) * YNET_COUT_PAD;
    return rp * K * K * cp;
}

int ynet_pack_weight(const float* w, float* wp, int cout, int cin, int K, int mode, void* stream) {
    YNET_REQUIRE(w && wp, "pack_weight: null pointer");
    YNET_REQUIRE(mode == 0 || mode == 1, "pack_weight: mode must be 0 (forward) or 1 (dgrad)");
    YNET_REQUIRE(cout > 0 && cin > 0 && (K == 1 || K == 3 || K == 5), "pack_weight: bad shape %d %d %d", cout, cin, K);
    const int rows = mode == 0 ? cin : cout, cols = mode == 0 ? cout : cin;
    const int rp = ceil_div(rows, YNET_CIN_PAD) * YNET_CIN_PAD + YNET_CIN_PAD, cp = ceil_div(cols, YNET_COUT_PAD) * YNET_COUT_PAD;
    const long long n = (long long)rp * K * K * cp;
    const int grid = (int)((n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256);
    hipLaunchKernelGGL(pack_weight_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, wp, cout, cin, K * K,
                       mode, rows, cols, rp, cp);
    return ynet_check_launch("pack_weight");
}

// y[dst...] = [relu](conv(cat(src...) [masked], wp) + bias); cin = sum of source channels,
// cout = sum of destination channels.  See include/ynet_hip.h.
// Workspace (floats) that lets ynet_conv2d split the input-channel loop of a small-map launch over
// more workgroups; 0 when the problem is large enough not to need it.
long long ynet_conv2d_workspace_floats(int B, int H, int W, int cout) {
    if ((W & 3) != 0 || (long long)B * H * W > 64 * 1024) return 0;     // up to 32 x 32^2 or 64 x 16^2 ...
    return 8ll * B * cout * H * W;
}

static int conv2d_impl(const float* const* src, const int* src_c, const long long* src_bs, const int* src_bmod, int nsrc,
                       const float* mask, long long mask_bs, const float* wp, const float* bias,
                       float* const* dst, const int* dst_c, const long long* dst_bs, int ndst,
                       int B, int H, int W, int K, int relu, float* workspace, long long workspace_floats,
                       const float* addend, long long addend_bs, int addend_bmod, void* stream,
                       const float* emask = nullptr, long long emask_bs = 0, float* pool = nullptr, long long pool_bs = 0,
                       unsigned* bits_out = nullptr, const unsigned* bits_in = nullptr) {
    YNET_REQUIRE(nsrc >= 1 && nsrc <= YNET_MAX_SRC && ndst >= 1 && ndst <= YNET_MAX_SRC,
                 "conv2d: 1..%d sources/destinations supported (got %d/%d)", YNET_MAX_SRC, nsrc, ndst);
    YNET_REQUIRE(B > 0 && H > 0 && W > 0, "conv2d: empty problem B=%d H=%d W=%d", B, H, W);
    YNET_REQUIRE(wp != nullptr, "conv2d: packed filter is null");
    YNET_REQUIRE(mask == nullptr || nsrc == 1, "conv2d: a ReLU mask needs a single source");
    ConvArgs a{};
    a.nsrc = nsrc;
    a.cin = 0;
    for (int i = 0; i < nsrc; ++i) {
        YNET_REQUIRE(src[i] != nullptr && src_c[i] > 0, "conv2d: source %d is null/empty", i);
        a.src[i] = YSrc{src[i], src_c[i], src_bs[i], src_bmod ? src_bmod[i] : 0};
        YNET_REQUIRE(a.src[i].bmod >= 0, "conv2d: negative batch modulus");
        a.cin += src_c[i];
    }
    a.ndst = ndst;
    a.cout = 0;
    for (int i = 0; i < ndst; ++i) {
        YNET_REQUIRE(dst_c[i] > 0, "conv2d: destination %d has no channels", i);
        a.dst[i] = YDst{dst[i], dst_c[i], dst_bs[i]};
        a.cout += dst_c[i];
    }
    // trailing destinations that are not wanted need not be computed at all
    while (a.ndst > 1 && a.dst[a.ndst - 1].p == nullptr) {
        a.cout -= a.dst[a.ndst - 1].c;
        --a.ndst;
    }
    {   // the packed filter was padded for the FULL cout
        int full = 0;
        for (int i = 0; i < ndst; ++i) full += dst_c[i];
        a.cout_pad = ceil_div(full, YNET_COUT_PAD) * YNET_COUT_PAD;
    }
    a.mask = mask;
    a.mask_bs = mask_bs;
    a.addend = addend;
    a.addend_bs = addend_bs;
    a.addend_bmod = addend_bmod;
    a.pool = pool;
    a.pool_bs = pool_bs;
    if (pool != nullptr) {
        YNET_REQUIRE(a.ndst == 1 && a.dst[0].p != nullptr && mask == nullptr && addend == nullptr && emask == nullptr, "conv2d_pool: one destination, no mask / additive term");
        YNET_REQUIRE((H & 1) == 0 && (W & 1) == 0 && (reinterpret_cast<uintptr_t>(pool) & 7) == 0 && (pool_bs & 1) == 0, "conv2d_pool: even H, W and an 8-byte aligned pooled output");
    }
    a.bits_out = bits_out;
    a.bits_in = bits_in;
    if (bits_out != nullptr || bits_in != nullptr) {
        YNET_REQUIRE(a.ndst == 1 && a.dst[0].p != nullptr && addend == nullptr && emask == nullptr && pool == nullptr && !(bits_out && bits_in),
                     "conv2d (bit mask): one destination, no additive term / float mask / pooled copy");
        YNET_REQUIRE((reinterpret_cast<uintptr_t>(bits_out ? bits_out : const_cast<unsigned*>(bits_in)) & 3) == 0, "conv2d (bit mask): unaligned mask words");
    }
    a.emask = emask;
    a.emask_bs = emask_bs;
    if (emask != nullptr) {
        YNET_REQUIRE(a.ndst == 1 && a.dst[0].p != nullptr && addend == nullptr, "conv2d: the output-side ReLU mask needs exactly one destination");
        YNET_REQUIRE((reinterpret_cast<uintptr_t>(emask) & 15) == 0 && (emask_bs & 3) == 0, "conv2d_dgrad_relu: relu_of (the output-side ReLU mask) must be 16-byte aligned with a batch stride that is a multiple of 4 floats");
    }
    a.wp = wp;
    a.bias = bias;
    a.B = B;
    a.H = H;
    a.W = W;
    a.relu = relu;
    a.partial = ((W & 3) == 0 && workspace_floats > 0) ? workspace : nullptr;
    a.partial_cap = workspace_floats;
    a.vec_store = (W % 4 == 0) ? 1 : 0;
    for (int i = 0; i < a.ndst; ++i)
        if (a.dst[i].p && ((reinterpret_cast<uintptr_t>(a.dst[i].p) & 15) || (a.dst[i].bs & 3))) a.vec_store = 0;
    a.vec_load = (W % 4 == 0) ? 1 : 0;
    for (int i = 0; i < a.nsrc; ++i)
        if ((reinterpret_cast<uintptr_t>(a.src[i].p) & 15) || (a.src[i].bs & 3)) a.vec_load = 0;
    if (mask && ((reinterpret_cast<uintptr_t>(mask) & 15) || (mask_bs & 3))) a.vec_load = 0;
    if ((W % 4) == 0 && (pool != nullptr || bits_out != nullptr || bits_in != nullptr || addend != nullptr)) {
        // The pooled copy, the 1-bit masks and the additive term exist in the LDS-DMA kernels only.  An operand off a 16-byte boundary would
        // send the call to the register-staged tiles, which have no such epilogue: say which operand it is.
        const char* what = pool ? "conv2d_pool" : (addend ? "conv2d_add" : "conv2d (bit mask)");
        for (int i = 0; i < a.nsrc; ++i)
            YNET_REQUIRE(!(reinterpret_cast<uintptr_t>(a.src[i].p) & 15) && !(a.src[i].bs & 3),
                         "%s: source %d must be 16-byte aligned with a batch stride that is a multiple of 4 floats", what, i);
        YNET_REQUIRE(!mask || (!(reinterpret_cast<uintptr_t>(mask) & 15) && !(mask_bs & 3)),
                     "%s: the mask must be 16-byte aligned with a batch stride that is a multiple of 4 floats", what);
        YNET_REQUIRE(!(reinterpret_cast<uintptr_t>(a.dst[0].p) & 15) && !(a.dst[0].bs & 3),
                     "%s: the destination must be 16-byte aligned with a batch stride that is a multiple of 4 floats", what);
        YNET_REQUIRE(!addend || (!(reinterpret_cast<uintptr_t>(addend) & 15) && !(addend_bs & 3)),
                     "%s: the additive term (addend) must be 16-byte aligned with an image stride that is a multiple of 4 floats", what);
    }
    return conv_dispatch(a, K, (hipStream_t)stream);
}

int ynet_conv2d(const float* const* src, const int* src_c, const long long* src_bs, const int* src_bmod, int nsrc,
                const float* mask, long long mask_bs, const float* wp, const float* bias,
                float* const* dst, const int* dst_c, const long long* dst_bs, int ndst,
                int B, int H, int W, int K, int relu, float* workspace, long long workspace_floats,
                void* stream) {
    return conv2d_impl(src, src_c, src_bs, src_bmod, nsrc, mask, mask_bs, wp, bias, dst, dst_c, dst_bs, ndst, B, H, W, K, relu,
                       workspace, workspace_floats, nullptr, 0, 0, stream);
}

// ynet_conv2d as a data gradient whose result is written THROUGH the ReLU backward of the layer below: dx = relu_of > 0 ?
// conv(dy [masked where mask <= 0], wp) : 0, relu_of = that layer's post-ReLU output = this convolution's forward input.
int ynet_conv2d_dgrad_relu(const float* dy, int dy_c, long long dy_bs, const float* mask, long long mask_bs, const float* wp,
                           float* dx, int dx_c, long long dx_bs, const float* relu_of, long long relu_of_bs,
                           int B, int H, int W, int K, float* workspace, long long workspace_floats, void* stream) {
    YNET_REQUIRE(dy != nullptr && dx != nullptr && relu_of != nullptr, "conv2d_dgrad_relu: null pointer");
    const float* srcs[1] = {dy};
    const int sc[1] = {dy_c};
    const long long sb[1] = {dy_bs};
    float* dsts[1] = {dx};
    const int dc[1] = {dx_c};
    const long long db[1] = {dx_bs};
    return conv2d_impl(srcs, sc, sb, nullptr, 1, mask, mask_bs, wp, nullptr, dsts, dc, db, 1, B, H, W, K, 0, workspace, workspace_floats,
                       nullptr, 0, 0, stream, relu_of, relu_of_bs);
}

// Words (uint32) of the 1-bit activation mask a ReLU convolution with this OUTPUT shape writes next to its output
// (ynet_conv2d_relu_bits) and the data gradient of the following convolution applies to ITS output, which has that same
// shape (ynet_conv2d_dgrad_relu_bits); 0: this shape is not served (then ynet_conv2d + ynet_conv2d_dgrad_relu with the float
// activation).  Both launches tile the [B, cout, H, W] tensor identically (the tiling is a function of B, H, W, cout, K only),
// and the mask lives in the register layout of those tiles: [tile][256 lanes][ceil(tiles * rows * 8 / 32)].
long long ynet_conv2d_relu_bits_words(int B, int H, int W, int cout, int K) {
    const DirectPlan p = shape_plan(B, H, W, cout, K);
    if (!conv_gates().relu_bits || p.gen != GEN_DMA) return 0;
    const long long tiles = (long long)ceil_div(W, 32) * ceil_div(H, 4 * p.rows) * ceil_div(cout, p.cb) * B;
    return tiles * 256 * ((p.tiles * p.rows * 8 + 31) / 32);
}

// relu(conv(cat(src...), wp) + bias) -> dst, and the 1-bit mask (dst > 0) -> bits [ynet_conv2d_relu_bits_words(...)]
int ynet_conv2d_relu_bits(const float* const* src, const int* src_c, const long long* src_bs, int nsrc, const float* wp, const float* bias,
                          float* dst, int cout, long long dst_bs, unsigned* bits, int B, int H, int W, int K, void* stream) {
    YNET_REQUIRE(dst != nullptr && bits != nullptr, "conv2d_relu_bits: null destination");
    YNET_REQUIRE(ynet_conv2d_relu_bits_words(B, H, W, cout, K) > 0, "conv2d_relu_bits: shape B=%d %dx%d cout=%d K=%d is not served (ask ynet_conv2d_relu_bits_words)", B, H, W, cout, K);
    float* dsts[1] = {dst};
    const int dc[1] = {cout};
    const long long db[1] = {dst_bs};
    return conv2d_impl(src, src_c, src_bs, nullptr, nsrc, nullptr, 0, wp, bias, dsts, dc, db, 1, B, H, W, K, 1, nullptr, 0,
                       nullptr, 0, 0, stream, nullptr, 0, nullptr, 0, bits, nullptr);
}

// ynet_conv2d_dgrad_relu with the activation of the layer below given as the bit mask its forward convolution wrote:
// dx = bit ? conv(dy [masked where mask <= 0], wp) : 0
int ynet_conv2d_dgrad_relu_bits(const float* dy, int dy_c, long long dy_bs, const float* mask, long long mask_bs, const float* wp,
                                float* dx, int dx_c, long long dx_bs, const unsigned* bits, int B, int H, int W, int K, void* stream) {
    YNET_REQUIRE(dy != nullptr && dx != nullptr && bits != nullptr, "conv2d_dgrad_relu_bits: null pointer");
    YNET_REQUIRE(ynet_conv2d_relu_bits_words(B, H, W, dx_c, K) > 0, "conv2d_dgrad_relu_bits: shape B=%d %dx%d channels=%d K=%d is not served (ask ynet_conv2d_relu_bits_words)", B, H, W, dx_c, K);
    const float* srcs[1] = {dy};
    const int sc[1] = {dy_c};
    const long long sb[1] = {dy_bs};
    float* dsts[1] = {dx};
    const int dc[1] = {dx_c};
    const long long db[1] = {dx_bs};
    return conv2d_impl(srcs, sc, sb, nullptr, 1, mask, mask_bs, wp, nullptr, dsts, dc, db, 1, B, H, W, K, 0, nullptr, 0,
                       nullptr, 0, 0, stream, nullptr, 0, nullptr, 0, nullptr, bits);
}

// ynet_conv2d with one destination + its 2 x 2 max-pooled copy (MaxPool2d(2, 2) of the next encoder stage, models/ynet.py:202,215)
// written by the same epilogue.  ynet_conv2d_pool_supported: the shapes that take it (3x3, two-row tiles: the large maps, where the
// stand-alone pool is a 60 us pass on the forward's critical path).
int ynet_conv2d_pool_supported(int B, int H, int W, int cout, int K) {
    return ((H | W) & 1) == 0 && shape_plan(B, H, W, cout, K).gen == GEN_DMA;
}

int ynet_conv2d_pool(const float* const* src, const int* src_c, const long long* src_bs, int nsrc, const float* wp, const float* bias,
                     float* dst, int cout, long long dst_bs, float* pooled, long long pooled_bs,
                     int B, int H, int W, int K, int relu, void* stream) {
    YNET_REQUIRE(dst != nullptr && pooled != nullptr, "conv2d_pool: null destination");
    // (refused before anything is launched; conv_dispatch holds the plan of the actual call, operand alignment included, to the same rule)
    YNET_REQUIRE(ynet_conv2d_pool_supported(B, H, W, cout, K), "conv2d_pool: shape B=%d %dx%d cout=%d is not served by the pooling epilogue (ask ynet_conv2d_pool_supported)", B, H, W, cout);
    float* dsts[1] = {dst};
    const int dc[1] = {cout};
    const long long db[1] = {dst_bs};
    return conv2d_impl(src, src_c, src_bs, nullptr, nsrc, nullptr, 0, wp, bias, dsts, dc, db, 1, B, H, W, K, relu, nullptr, 0,
                       nullptr, 0, 0, stream, nullptr, 0, pooled, pooled_bs);
}

// 1 if ynet_conv2d_dgrad_relu applies the mask inside the convolution kernel for this problem (3x3 on a map large enough for
// two-row units); elsewhere it is still correct but adds a pass over dx -- callers keep the consumer-side mask there
int ynet_conv2d_dgrad_relu_supported(int B, int H, int W, int dx_c, int K) {
    return shape_plan(B, H, W, dx_c, K).gen == GEN_DMA;
}

// 1 if ynet_conv2d_add serves this problem (3x3, Cout 17..32 or 49..64, W % 4 == 0, a map large enough for two-row units)
int ynet_conv2d_add_supported(int B, int H, int W, int cout, int K) {
    return shape_plan(B, H, W, cout, K, true).gen == GEN_DMA;
}

// y = [relu](conv(cat(src...), wp) + bias + addend[b % addend_bmod]): ynet_conv2d with one destination, no mask, plus a
// precomputed term [images][cout][H][W] (batch stride addend_bs, addend_bmod > 0: that many images repeating along the
// batch) -- the part of the convolution over inputs that repeat along the batch, computed once (utils/evaluate.py: the K
// goal samples of a trajectory share its encoder features).
int ynet_conv2d_add(const float* const* src, const int* src_c, const long long* src_bs, const int* src_bmod, int nsrc,
                    const float* wp, const float* bias, float* dst, int cout, long long dst_bs,
                    int B, int H, int W, int K, int relu, const float* addend, long long addend_bs, int addend_bmod,
                    void* stream) {
    YNET_REQUIRE(addend != nullptr && dst != nullptr && addend_bmod >= 0, "conv2d_add: null pointer / negative modulus");
    float* dsts[1] = {dst};
    const int dc[1] = {cout};
    const long long db[1] = {dst_bs};
    return conv2d_impl(src, src_c, src_bs, src_bmod, nsrc, nullptr, 0, wp, bias, dsts, dc, db, 1, B, H, W, K, relu, nullptr, 0,
                       addend, addend_bs, addend_bmod, stream);
}

}  // extern "C"
