// kz_board_conv_i8.hip — per-layer 3x3 convolution on the i8 matrix cores for the ResTowers the one-launch int8 tower
// (kz_tower_i8.hip) cannot hold: Go 19x19 / 13x13, 9x9 at 256 channels, towers above 256 channels, of 64 or fewer, of
// 129 .. 192 ("board_conv_i8", KZ_DTYPE_INT8_ANY where dtype 5 refuses the shape).  The arithmetic is the int8 contract of
// include/kz_hip.h ("int8 calibration"), stated per convolution: it does not depend on the geometry.
//
// The board-tile organisation of kz_board_conv.hip with its LDS image taken over byte for byte: a workgroup keeps whole
// boards (Geometry: bpw boards of tpb tiles of 16 pixel rows, 24 tiles) with a zero halo in LDS, a tap is a constant byte
// offset, 256 threads = 4 waves = 4 row quarters of 6 tiles x the workgroup's 64 output channels, two workgroups per CU, the
// XCD-aware 1-D grid.  One chunk of that image is 128 bytes per pixel in two planes of 64 B + 16 B pad: 64 f16 channels
// there, 128 INT8 channels here.  Two v_mfma_i32_16x16x64_i8 k-steps per tap (KPC = 18, as there), each lane's 16 bytes the
// sixteen channels 64 (kq & 1) + 32 ks + 16 (kq >> 1) + j of the chunk: lane groups kq and kq + 1 read the two planes at the
// same row offset, the sixteen rows of a tile fall on sixteen different 16-byte slots of the 256-byte bank row — the rule of
// the f16 kernel holds for 1-byte elements because the BYTES of a fragment read are the same.
//
// What is NOT taken over: the weight ring that doubles as the staging buffer, the early weight step, the
// priority pairing of the CU's two workgroups and the padding-tile skip.  A chunk is staged between two barriers, the weights
// of a k-step are requested one k-step ahead, and the compiler schedules the rest; the CU's second workgroup covers the
// staging of the first.
//
// Tensors: the int8 images X8 / Y8 are [boards*hw][C8] bytes, C8 = the tower's channels widened to the next multiple of 128
// (a chunk) with all-zero filters (f = 0, bias 0: the widened channels of every image are 0); the f16 residual stream beside
// them is the f16 engine's [boards*hw][cp] rows.  Two instances of one body:
//   kz_board_conv_i8       a block convolution.  t = (float)acc; v = t * mult[oc] + bias[oc] (one rounding); ReLU.
//                          conv A: Y8 = quant(v, e_mid).  conv B: v += (float)x in f32, after the ReLU; x = f16(v) and
//                          X8 = quant(v, e_next), both from the same f32 v.  The last conv B: final BN in f32, f16 rows only.
//   kz_board_conv_i8_stem  the f16 board-tile stem (f16 operands, f32 accumulation from the bias, chunks of 64 f16 input
//                          planes) with two stores from one f32 v: the stream's f16(v) and X8 = quant(v, e_0).
// quant(v, e) = clamp(rne(v * 2^-e), -127, 127); it never takes f16(v).
// The results leave through an output tile in LDS (the image is dead by then) as whole 16-byte pieces of 128-byte (f16) and
// 64-byte (int8) row segments: f16 tile rows of 144 B, int8 tile rows of 80 B.  A wave's ds_write_b32 of an int8 tile — lane
// (fr, kq) writes word 20 fr + kq (+ 4 nt) — puts two lanes on every bank, the minimum for 256 bytes; its ds_write_b64 of an
// f16 tile (words 36 fr + 2 kq) four, the minimum for 512.
#include <cstdint>
#include <type_traits>

#include "kz_board_conv_i8_pack.hpp"
#include "kz_kernels.hpp"
#include "kz_launch.hpp"

namespace kz {

namespace {

typedef _Float16 h16;
typedef h16 h16x8 __attribute__((ext_vector_type(8)));
typedef h16 h16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int MT = 24;            // 16-row tiles per workgroup (kz_board_conv.hip's)
constexpr int ROWS = MT * 16;     // 384
constexpr int OCW = 64;           // output channels per workgroup
constexpr int CHB = 128;          // bytes of a pixel row per staged chunk: 128 int8 or 64 f16 channels
constexpr int PRS = 64 + 16;      // plane row stride
constexpr int KPC = 18;           // k-steps per chunk: 9 taps x 2
constexpr int MTW = MT / 4;       // tiles per wave
constexpr int ORS16 = OCW * 2 + 16, ORS8 = OCW + 16;  // row strides of the f16 and the int8 output tile

struct BoardConvI8Dev {
    const void *x;          // I8: [pixels][C8] int8; stem: [pixels][cin] f16
    const uint4 *w;         // fragment-packed: [quarter][chunk][tap][ks 2][nt 4][lane 64] x 16 B
    const float *bias, *mult, *post_scale, *post_shift;  // [C8]
    const h16 *res;         // optional f16 residual [pixels][cp]
    h16 *y16;               // optional f16 rows out [pixels][cp]
    signed char *y8;        // optional int8 image out [pixels][C8]
    float qscale;           // 2^-e of y8's site
    int bytes_x, ldx_b;     // size and row bytes of x
    int bytes16, ld16_b;    // of the f16 stream (res and y16)
    int bytes8, ld8_b;      // of y8
    int boards, h, w_, hw, tpb, bpw, chunks, relu, groups, nq;
    unsigned inv_tpb, inv_w, inv_nhb, inv_10;
    int pitch, plane, line16, board16;
};

__device__ __forceinline__ u32x4 lds_frag(int addr) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const u32x4 __attribute__((address_space(3))) * lds_cptr;
    return *(lds_cptr)(unsigned)addr;
#else
    (void)addr;
    return u32x4{};
#endif
}

// clamp(rne(v * qs), -127, 127) of four values as the four bytes of a word, the first channel lowest (kz_tower_i8.hip's)
__device__ __forceinline__ int quant4(f32x4 v, float qs) {
    int r = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float q = fminf(fmaxf(__builtin_rintf(v[j] * qs), -127.0f), 127.0f);
        r |= ((int)q & 0xff) << (8 * j);
    }
    return r;
}

template <bool I8>
__device__ __forceinline__ void board_conv_i8_body(const BoardConvI8Dev &a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x;
    const int wr = __builtin_amdgcn_readfirstlane(tid >> 6);  // the wave = a row quarter
    const int lane = tid & 63;
    const int fr = lane & 15, kq = lane >> 4;
    // XCD-aware order (kz_board_conv.hip): the nq channel quarters of a board group take consecutive slots of one XCD
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int nquarter = slot % a.nq, group = (slot / a.nq) * 8 + xcd;
    if (group >= a.groups) return;
    const int board0 = group * a.bpw;

    // slot i of a thread = tile row trow + 32 i, 16-byte piece `piece` of the row's 128 bytes: the f16 kernel's map (a
    // ds_write_b128 group of eight lanes = pieces 0..3 of rows r and r + 4)
    const int piece = (tid & 3) | ((tid >> 3) & 4);
    const int trow = ((tid >> 3) & 3) | (tid & 4) | ((tid >> 6) << 3);
    const int ls_piece = (piece >> 2) * a.plane + (piece & 3) * 16;
    // tile row r -> pixel index in the batch and 16-byte slot of the pixel row in the image; false for a padding row or a
    // board beyond the batch
    auto locate = [&](int r, int &pix, int &irow) __attribute__((always_inline)) {
        const int b = (int)(__umul24((unsigned)(r >> 4), a.inv_tpb) >> 16);
        const int q = r - (int)__umul24((unsigned)b, (unsigned)a.tpb * 16u);
        const int yy = (int)(__umul24((unsigned)q, a.inv_w) >> 16);
        irow = (int)__umul24((unsigned)b, (unsigned)a.board16) + (int)__umul24((unsigned)(yy + 1), (unsigned)a.line16) +
               (q - (int)__umul24((unsigned)yy, (unsigned)a.w_) + 1) * 5;
        pix = (int)(__umul24((unsigned)(board0 + b), (unsigned)a.hw) + (unsigned)q);
        return b < a.bpw && q < a.hw && board0 + b < a.boards;
    };
    const auto xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.x), 0, a.bytes_x, 0x00020000);
    // a chunk of the image: 12 coalesced 16-byte pieces per thread (an offset of -1 is out of range: the load returns zeros
    // and touches no memory), then into the pixel rows — never into the halo
    auto stage = [&](int chunk) __attribute__((always_inline)) {
        u32x4 v[12];
        int irows[12];
#pragma unroll
        for (int i = 0; i < 12; i++) {
            int pix;
            const bool ok = locate(trow + i * 32, pix, irows[i]);
            if (!ok) irows[i] = -1;
            v[i] = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, ok ? (int)__umul24((unsigned)pix, (unsigned)a.ldx_b) + chunk * CHB + piece * 16 : -1, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 12; i++)
            if (irows[i] >= 0) *reinterpret_cast<u32x4 *>(lds + irows[i] * 16 + ls_piece) = v[i];
    };

    // zero the halo once (kz_board_conv.hip: per board and plane the line above, the line below and per pixel line its left
    // and right halo rows)
    {
        const int nhb = a.line16 + 5 * (a.pitch + 1) + 10 * a.h;
        for (int id = tid; id < 2 * a.bpw * nhb; id += 256) {
            const int pb = (int)__umulhi((unsigned)id, a.inv_nhb), k = id - pb * nhb;
            const int pl = pb >= a.bpw ? 1 : 0, b = pb - pl * a.bpw;
            int slot16;
            if (k < a.line16) {
                slot16 = k;
            } else if (k < a.line16 + 5 * (a.pitch + 1)) {
                slot16 = (a.h + 1) * a.line16 + (k - a.line16);
            } else {
                const int kk = k - a.line16 - 5 * (a.pitch + 1);
                const int y = (int)(((unsigned)kk * a.inv_10) >> 16), pc = kk - y * 10;
                slot16 = (y + 1) * a.line16 + (pc < 5 ? pc : a.pitch * 5 + pc - 5);
            }
            *reinterpret_cast<uint4 *>(lds + pl * a.plane + (b * a.board16 + slot16) * 16) = make_uint4(0, 0, 0, 0);
        }
    }

    // centre-tap LDS address of this lane's fragment row per tile; a lane without a pixel reads pixel (0, 0) of board 0 (its
    // outputs are never stored)
    int T0[MTW];
#pragma unroll
    for (int i = 0; i < MTW; i++) {
        int pix, irow;
        const bool valid = locate((wr * MTW + i) * 16 + fr, pix, irow);
        T0[i] = (valid ? irow : a.line16 + 5) * 16 + (kq & 1) * a.plane + (kq >> 1) * 16;
    }

    typedef std::conditional_t<I8, i32x4, f32x4> acc_t;
    acc_t acc[4][MTW];
    const int oc0 = nquarter * OCW + kq * 4;  // + nt * 16: this lane's four output channels of tile column nt
#pragma unroll
    for (int nt = 0; nt < 4; nt++) {
        acc_t z{};
        if constexpr (!I8) z = *reinterpret_cast<const f32x4 *>(a.bias + oc0 + nt * 16);  // (the f16 stem sums from the bias)
#pragma unroll
        for (int i = 0; i < MTW; i++) acc[nt][i] = z;
    }

    for (int chunk = 0; chunk < a.chunks; chunk++) {
        if (chunk) __syncthreads();  // every wave is done with the previous chunk's fragments
        stage(chunk);
        __syncthreads();
        const uint4 *wp = a.w + ((size_t)(nquarter * a.chunks + chunk) * KPC) * 256 + lane;
        int pitch_b = a.line16 * 16;  // bytes from a line to the next (behind a barrier: the tap rows are not hoisted and spilled)
        asm volatile("" : "+s"(pitch_b));
        uint4 wcur[4], wnxt[4];
#pragma unroll
        for (int nt = 0; nt < 4; nt++) wcur[nt] = wp[nt * 64];
#pragma unroll
        for (int s = 0; s < KPC; s++) {
            const int tap = s >> 1, ks = s & 1;
            if (s + 1 < KPC) {
#pragma unroll
                for (int nt = 0; nt < 4; nt++) wnxt[nt] = wp[(size_t)(s + 1) * 256 + nt * 64];
            }
            const int off = (tap / 3 - 1) * pitch_b + (tap % 3 - 1) * PRS + ks * 32;
#pragma unroll
            for (int i = 0; i < MTW; i++) {
                const u32x4 bf = lds_frag(T0[i] + off);
#pragma unroll
                for (int nt = 0; nt < 4; nt++) {
                    if constexpr (I8)
                        acc[nt][i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, wcur[nt]), __builtin_bit_cast(i32x4, bf), acc[nt][i], 0, 0, 0);
                    else
                        acc[nt][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, wcur[nt]), __builtin_bit_cast(h16x8, bf), acc[nt][i], 0, 0, 0);
                }
            }
#pragma unroll
            for (int nt = 0; nt < 4; nt++) wcur[nt] = wnxt[nt];
        }
    }

    // ---- epilogue: one f32 v per element; everything stored is made from it ----
    const bool with_res = I8 && a.res != nullptr;
    const auto rrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<h16 *>(with_res ? a.res : a.y16), 0, with_res ? a.bytes16 : 0, 0x00020000);
    // the 12 slots of a thread in the f16 stream: this workgroup's 64 channels of a row are 128 bytes; a piece beyond the
    // stream's cp channels (the tower widened to C8) is out of range, like a padding row
    int po16[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        int pix, irow;
        const bool ok = locate(trow + i * 32, pix, irow);
        const int col = nquarter * OCW * 2 + piece * 16;
        po16[i] = ok && col < a.ld16_b ? (int)__umul24((unsigned)pix, (unsigned)a.ld16_b) + col : -1;
    }
    u32x4 rv[12];
    if (with_res) {
#pragma unroll
        for (int i = 0; i < 12; i++) rv[i] = __builtin_amdgcn_raw_buffer_load_b128(rrsrc, po16[i], 0, 0);
    }
    f32x4 v[4][MTW];
#pragma unroll
    for (int nt = 0; nt < 4; nt++) {
        f32x4 mu = f32x4{1.f, 1.f, 1.f, 1.f}, bi = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (I8) {
            mu = *reinterpret_cast<const f32x4 *>(a.mult + oc0 + nt * 16);
            bi = *reinterpret_cast<const f32x4 *>(a.bias + oc0 + nt * 16);
        }
#pragma unroll
        for (int i = 0; i < MTW; i++) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float t;
                if constexpr (I8) t = __builtin_fmaf((float)acc[nt][i][j], mu[j], bi[j]);  // (the product is exact: one rounding)
                else t = acc[nt][i][j];
                v[nt][i][j] = a.relu ? fmaxf(t, 0.0f) : t;
            }
        }
    }
    __syncthreads();  // every wave is done with the last chunk's fragments: the image is dead, the output tiles take its place
    if (with_res) {
#pragma unroll
        for (int i = 0; i < 12; i++) *reinterpret_cast<u32x4 *>(lds + (trow + i * 32) * ORS16 + piece * 16) = rv[i];
        __syncthreads();
#pragma unroll
        for (int nt = 0; nt < 4; nt++)
#pragma unroll
            for (int i = 0; i < MTW; i++) {
                const h16x4 r = *reinterpret_cast<const h16x4 *>(lds + ((wr * MTW + i) * 16 + fr) * ORS16 + (nt * 16 + kq * 4) * 2);
#pragma unroll
                for (int j = 0; j < 4; j++) v[nt][i][j] += (float)r[j];  // added in f32, AFTER the ReLU
            }
    }
    if (a.post_scale) {
#pragma unroll
        for (int nt = 0; nt < 4; nt++) {
            const f32x4 ps = *reinterpret_cast<const f32x4 *>(a.post_scale + oc0 + nt * 16), pt = *reinterpret_cast<const f32x4 *>(a.post_shift + oc0 + nt * 16);
#pragma unroll
            for (int i = 0; i < MTW; i++) v[nt][i] = v[nt][i] * ps + pt;
        }
    }
    if (a.y16) {
        // each lane rewrites the 8 bytes it owns (with a residual: the ones it has just read), then whole rows leave
#pragma unroll
        for (int nt = 0; nt < 4; nt++)
#pragma unroll
            for (int i = 0; i < MTW; i++)
                *reinterpret_cast<h16x4 *>(lds + ((wr * MTW + i) * 16 + fr) * ORS16 + (nt * 16 + kq * 4) * 2) =
                    h16x4{(h16)v[nt][i][0], (h16)v[nt][i][1], (h16)v[nt][i][2], (h16)v[nt][i][3]};
        __syncthreads();
        const auto yrsrc = __builtin_amdgcn_make_buffer_rsrc(a.y16, 0, a.bytes16, 0x00020000);
#pragma unroll
        for (int i = 0; i < 12; i++)  // a padding row's store is out of range and dropped
            __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4 *>(lds + (trow + i * 32) * ORS16 + piece * 16), yrsrc, po16[i], 0, 0);
    }
    if (a.y8) {
        if (a.y16) __syncthreads();  // the f16 tile has been read back
#pragma unroll
        for (int nt = 0; nt < 4; nt++)
#pragma unroll
            for (int i = 0; i < MTW; i++)
                *reinterpret_cast<int *>(lds + ((wr * MTW + i) * 16 + fr) * ORS8 + nt * 16 + kq * 4) = quant4(v[nt][i], a.qscale);
        __syncthreads();
        // an int8 tile row is 64 bytes, four pieces: thread -> (row = tid / 4 + 64 k, piece = tid % 4)
        const auto qrsrc = __builtin_amdgcn_make_buffer_rsrc(a.y8, 0, a.bytes8, 0x00020000);
#pragma unroll
        for (int k = 0; k < ROWS / 64; k++) {
            const int r = (tid >> 2) + k * 64, p = tid & 3;
            int pix, irow;
            const bool ok = locate(r, pix, irow);
            __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4 *>(lds + r * ORS8 + p * 16), qrsrc,
                                                   ok ? (int)__umul24((unsigned)pix, (unsigned)a.ld8_b) + nquarter * OCW + p * 16 : -1, 0, 0);
        }
    }
}

__global__ __launch_bounds__(256, 2) void kz_board_conv_i8(BoardConvI8Dev a) { board_conv_i8_body<true>(a); }
__global__ __launch_bounds__(256, 2) void kz_board_conv_i8_stem(BoardConvI8Dev a) { board_conv_i8_body<false>(a); }

}  // namespace

int board_conv_i8_channels(int channels) { return (channels + CHB - 1) / CHB * CHB; }

bool board_conv_i8_supported(int h, int w, int channels) {
    return channels >= 1 && board_conv_i8_channels(channels) <= 512 && w <= 32 && h <= 32 && w >= 2 && h >= 2 && board_conv_geometry(h, w).bpw >= 1;
}

size_t board_conv_i8_weight_bytes(int cin8, int cout8) { return (size_t)9 * cin8 * cout8; }

void board_conv_i8_pack_weights(const int8_t *wq, int cout, int cin, int cout8, int cin8, int8_t *dst) {
    board_conv_i8_pack_weights_host(wq, cout, cin, cout8, cin8, dst);
}

void launch_board_conv_i8(const BoardConvI8Args &t, hipStream_t stream) {
    BoardConvI8Dev d;
    const size_t pixels = (size_t)t.boards * t.h * t.w;
    d.x = t.x;
    d.w = static_cast<const uint4 *>(t.weights);
    d.bias = t.bias;
    d.mult = t.mult;
    d.post_scale = t.post_scale;
    d.post_shift = t.post_shift;
    d.res = static_cast<const h16 *>(t.res);
    d.y16 = static_cast<h16 *>(t.y16);
    d.y8 = static_cast<signed char *>(t.y8);
    d.qscale = t.qscale;
    d.ldx_b = t.stem ? t.cin * 2 : t.cin;
    d.bytes_x = (int)(pixels * d.ldx_b);
    d.ld16_b = t.ld16 * 2;
    d.bytes16 = (int)(pixels * d.ld16_b);
    d.ld8_b = t.cout;
    d.bytes8 = (int)(pixels * d.ld8_b);
    d.boards = t.boards;
    d.h = t.h;
    d.w_ = t.w;
    d.hw = t.h * t.w;
    const BoardConvGeometry geo = board_conv_geometry(t.h, t.w);
    d.tpb = geo.tpb;
    d.bpw = geo.bpw;
    d.pitch = geo.pitch;
    d.line16 = geo.line16;
    d.board16 = geo.board16;
    d.plane = geo.plane;
    d.chunks = d.ldx_b / CHB;
    d.relu = t.relu;
    d.groups = (t.boards + d.bpw - 1) / d.bpw;
    d.nq = t.cout / OCW;
    d.inv_tpb = (65536u + (unsigned)geo.tpb - 1) / (unsigned)geo.tpb;
    d.inv_w = (65536u + (unsigned)t.w - 1) / (unsigned)t.w;
    const unsigned nhb = (unsigned)geo.line16 + 5 * ((unsigned)geo.pitch + 1) + 10 * (unsigned)t.h;
    d.inv_nhb = (unsigned)(((1ull << 32) + nhb - 1) / nhb);
    d.inv_10 = (65536u + 9) / 10;
    const int grid = ((d.groups + 7) / 8) * 8 * d.nq;
    // the image (two planes) or the larger output tile, whichever is longer — Geometry::rm_off
    static_assert(ROWS * ORS8 <= ROWS * ORS16, "the int8 tile lies inside the f16 tile's bytes");
    const int lds_bytes = geo.rm_off;
    if (t.stem) {
        allow_dynamic_lds<kz_board_conv_i8_stem>(160 * 1024);
        kz_board_conv_i8_stem<<<grid, 256, lds_bytes, stream>>>(d);
    } else {
        allow_dynamic_lds<kz_board_conv_i8>(160 * 1024);
        kz_board_conv_i8<<<grid, 256, lds_bytes, stream>>>(d);
    }
}

}  // namespace kz
