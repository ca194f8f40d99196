// kz_tower_i8.hip — the one-launch ResTower on the i8 matrix cores: "tower_resident_i8" (dtype 4 and 5, a calibrated model),
// and with the conv policy heads, the scalar head and decode_output behind it in the same launch "tower_resident_i8+heads"
// (dtype 5 where tower_i8_conv_heads_supported holds; the HEADS = 2 instances, described in front of the kernel).
//
// The organisation of the plain-f16 launch (kz_tower_pairs.hpp with SPLIT = false): 256 threads, each wave a quarter of the
// output channels; the residual stream and the mid activation live in LDS for the whole tower; the weights stream from L2
// straight into MFMA A-fragment registers through a ring that runs on across layer boundaries; im2col is LDS addressing, a
// tap outside the board reads an all-zero row; the board encode is fused.  What differs is the operand width of the block
// convolutions: v_mfma_i32_16x16x64_i8 takes the same 16 bytes per lane as the f16 instruction and multiplies 64 values of
// k with them, so a k-step is 64 input channels (G = C / 64 k-steps per tap) and the sums are exact integers.
//
// The arithmetic (include/kz_hip.h, "KZ_DTYPE_INT8"; every scale a power of two, so applying one is exact in f32):
//   quant(v, e) = clamp(rne(v * 2^-e), -127, 127) as int8 (v_rndne_f32; -128 is never produced)
//   a block convolution, per output element: acc = the i32 sum of wq * q over 9 taps x C (exact); t = (float)acc;
//     v = t * 2^(e_in + f_oc) + bias[oc] (the product is exact: one rounding); ReLU
//   conv A stores Y8 = quant(v, e_mid).  Conv B adds (float)X to v in f32, after the ReLU, and stores X = f16(v) and
//     X8 = quant(v, e_next), both from the same f32 v.  The last layer: ReLU, residual, final BN in f32, f16 rows out.
//   the stem stays in f16 (its inputs are bits and a few scalars; nine k-steps): X = f16(v), X8 = quant(v, e_0)
// LDS holds X as an f16 image (rows of 2 C + 16 bytes; only its own lane's slot is ever read back, by the residual add), and
// the two int8 images X8 and Y8, which the convolutions read.
//
// Bank conflicts of the int8 fragment reads (the rule of Geo's comment in kz_tower_pairs.hpp, re-derived for 1-byte elements).
// A ds_read_b128 is served in four groups of sixteen lanes, and a group mixes eight rows of lane group kq = 0 (or 2) with the
// OTHER eight rows of kq = 1 (or 3): its sixteen 16-byte pieces fall on sixteen different slots of the 256-byte bank row only
// if the pieces of kq and kq + 1 of the same row are a multiple of 256 B apart and rows advance by an odd number of slots.  An
// int8 row is C <= 256 bytes, so inside ONE row no two pieces are 256 B apart, at any C: an int8 image is always TWO planes —
// channels [0, C/2) and [C/2, C) of every row, rows of C/2 + 16 bytes (9 or 5 slots), the planes a multiple of 256 B apart —
// and lane group kq reads plane kq & 1 at (kq >> 1) * C/4 bytes.  Byte j of lane group kq in k-step ch is channel
// {0, C/2, C/4, 3C/4}[kq] + 16 ch + j: the f16 family's assignment with 16-byte pieces of 16 channels (tower_i8_pack_weights
// packs the weights to match; the k order of a sum is free as long as both operands agree).
#include <iterator>
#include <utility>

#include "kz_kernels.hpp"
#include "kz_launch.hpp"

namespace kz {

typedef _Float16 h16;
typedef h16 h16x8 __attribute__((ext_vector_type(8)));
typedef h16 h16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

namespace {

#include "kz_decode_dev.hpp"  // DecodeDev, decode_board_wave: decode_output as the last step of a launch with the heads inside
#include "kz_conv_heads.hpp"  // conv_heads_tail: the conv policy heads and the scalar head behind two images in LDS
#include "kz_encode_dev.hpp"  // encoded_plane: the board encode's one statement

// ---- which instance a shape takes: tiles of 16 pixel rows per workgroup = floor(16 NT / hw) whole boards packed densely ----
struct I8Row {
    int c, nt;
    bool conv_heads;    // compiled with the conv heads' tail (HEADS = 2)
    bool plain = true;  // compiled as the tower alone (HEADS = 0)
};
// 256 channels: one 8x8 board (or as many smaller ones as 64 rows hold), two; 128 channels: chess, one Go 9x9 board, two Ataxx
// 7x7 boards (which straddle tile boundaries), and the wide levels of the plain-f16 family (split_wide_tiles_for,
// kz_tower_pairs_shapes.hpp): two 8x8 boards in 8 tiles, two 9x9 in 11, four 7x7 or eight 5x5 in 13 — and three 9x9 (or four
// 8x8) in 16 WITH THE HEADS INSIDE only: the tower alone was measured slower in sixteen tiles than in eleven at every batch
// (DESIGN.md 6.2.3), so that instance does not exist.  (<256, 8> has no tail: its scratch would not fit behind 148 KB.)
constexpr I8Row I8_ROWS[] = {{256, 4, true}, {256, 8, false}, {128, 4, true},  {128, 6, true},  {128, 7, true},
                             {128, 8, true}, {128, 11, true}, {128, 13, true}, {128, 16, true, false}};

constexpr int i8_tiles_for(int hw, int channels) {
    if (channels == 256) return hw <= 64 ? 4 : 0;
    if (channels == 128) return hw * 2 <= 112 ? 7 : hw <= 64 ? 4 : hw <= 96 ? 6 : 0;
    return 0;
}
// Workgroups a wide level must fill before it is taken, measured (the smallest measured batch from which the
// level beat the next narrower one beyond the regions' spread).  The tower alone: 256 at 128 channels — at 128 workgroups, half
// the CUs, a launch takes 1.7 times as long —, 128 for the two-board instance at 256 channels, as before.  With the heads
// inside every workgroup pays its encode and decode round trips to host memory once, and fewer, fuller workgroups win earlier:
// 128, and 342 for sixteen tiles (Go 9x9 at batch 1024).
constexpr int I8_WIDE_WORKGROUPS_PLAIN_128 = 256, I8_WIDE_WORKGROUPS_PLAIN_256 = 128;
constexpr int I8_WIDE_WORKGROUPS_HEADS = 128, I8_WIDE_WORKGROUPS_HEADS_16 = 342;
// More boards per workgroup: the weight stream is read once per workgroup and layer, and a launch with the heads inside pays
// its host round trips once per workgroup.  256 channels: two 8x8 boards (the f16 chess launch's footprint), the tower alone.
// 128 channels: the levels of split_wide_tiles_for.  The widest level that `batch` fills with workgroups is taken.
// heads_cap: 0 = the tower alone; else the launch has the heads inside and takes no level of more than heads_cap tiles (the
// plan's: the widest level whose tail fits the LDS, tower_i8_conv_heads_wide_cap)
constexpr int i8_wide_tiles_for(int hw, int channels, int batch, int heads_cap = 0) {
    int levels[2] = {0, 0};
    if (channels == 256) levels[0] = hw == 64 && !heads_cap ? 8 : 0;
    else if (channels == 128) {
        if (hw == 64 || hw == 81) {
            levels[0] = heads_cap ? 16 : 0;
            levels[1] = hw == 64 ? 8 : 11;
        } else {
            levels[0] = (hw == 49 || hw == 25) ? 13 : 0;
        }
    }
    for (int nt : levels) {
        if (!nt || (heads_cap && nt > heads_cap)) continue;
        const int per = nt * 16 / hw;
        const int fill = heads_cap ? (nt == 16 ? I8_WIDE_WORKGROUPS_HEADS_16 : I8_WIDE_WORKGROUPS_HEADS)
                                   : channels == 256 ? I8_WIDE_WORKGROUPS_PLAIN_256 : I8_WIDE_WORKGROUPS_PLAIN_128;
        if ((batch + per - 1) / per >= fill) return nt;
    }
    return 0;
}
constexpr int i8_tiles(int hw, int channels, int wide_batch, int heads_cap = 0) {
    const int nt = wide_batch ? i8_wide_tiles_for(hw, channels, wide_batch, heads_cap) : 0;
    return nt ? nt : i8_tiles_for(hw, channels);
}
constexpr bool i8_has_row(int channels, int nt, bool conv_heads = false) {
    for (const I8Row &r : I8_ROWS)
        if (r.c == channels && r.nt == nt && (conv_heads ? r.conv_heads : r.plain)) return true;
    return false;
}
// every tile count a rule returns has its row, as the tower alone and under every cap with the heads inside — a rule edited
// past the table does not build.  (One constant per channel count: the whole sweep in one constant expression is past the
// compiler's step limit.)
constexpr bool i8_rules_have_rows(int c) {
    for (int hw = 1; hw <= 512; hw++) {
        const int narrow = i8_tiles_for(hw, c);
        if (narrow && !i8_has_row(c, narrow)) return false;
        for (int batch : {1, 255, 256, 1024, 4096, 1 << 20})
            for (int cap : {0, 8, 11, 13, 16}) {
                const int nt = i8_wide_tiles_for(hw, c, batch, cap);
                if (nt && (!i8_has_row(c, nt, cap != 0) || (cap && nt > cap))) return false;
            }
    }
    return true;
}
template <int C>
constexpr bool I8_RULES_HAVE_ROWS = i8_rules_have_rows(C);
static_assert(I8_RULES_HAVE_ROWS<64> && I8_RULES_HAVE_ROWS<128> && I8_RULES_HAVE_ROWS<192> && I8_RULES_HAVE_ROWS<256> &&
                  I8_RULES_HAVE_ROWS<320> && I8_RULES_HAVE_ROWS<384> && I8_RULES_HAVE_ROWS<448> && I8_RULES_HAVE_ROWS<512>,
              "i8_tiles_for / i8_wide_tiles_for return a tile count that has no instance");

constexpr int SG_MFMA = 0x8, SG_VMEM_READ = 0x20, SG_DS_READ = 0x100;

// LDS bytes of the launch's own images (GeoI8<C, NT>::LDS_BYTES restated for the host: launch() asserts the two agree) and what
// the conv heads' tail gets as scratch behind them: the plain-f16 launch's 16 KB, or what is left of a CU's 160 KB
constexpr int i8_own_lds_bytes(int channels, int nt) {
    const int rows = nt * 16, rs = channels / 2 + 16;
    const int q_off = (rows * (channels * 2 + 16) + 255) / 256 * 256, plane = (2 * rows * rs + 16 * rs + 255) / 256 * 256;
    return q_off + 2 * plane;
}
constexpr int i8_tail_scratch_bytes(int channels, int nt) {
    const int room = 160 * 1024 - i8_own_lds_bytes(channels, nt);
    return room < (int)F16_TAIL_SCRATCH_BYTES ? room : (int)F16_TAIL_SCRATCH_BYTES;
}

template <int C, int NT>
struct GeoI8 {
    static constexpr int ROWS = NT * 16;
    static constexpr int OT = C / 64;  // 16-channel output tiles per wave
    static constexpr int G = C / 64;   // k-steps per tap: 64 channels each
    static constexpr int XRS = C * 2 + 16;  // the f16 stream image: bytes per pixel row
    static constexpr int XIMG = ROWS * XRS;
    static constexpr int RS = C / 2 + 16;   // a plane's row of an int8 image: an odd number of 16-byte slots
    static_assert((RS / 16) % 2 == 1, "rows advance by an odd number of slots");
    static constexpr int IMG = ROWS * RS;   // (a multiple of 256: every image of a plane starts on a bank row)
    // a plane = [X8][Y8][16 all-zero rows]; the planes a multiple of 256 B apart, behind the f16 image
    static constexpr int X8 = 0, Y8 = IMG, Z8 = 2 * IMG;
    static constexpr int PLANE = (2 * IMG + 16 * RS + 255) / 256 * 256;
    static constexpr int Q_OFF = (XIMG + 255) / 256 * 256;
    static constexpr int LDS_BYTES = Q_OFF + 2 * PLANE;
    static constexpr int STEP = 4 * OT * 64;  // uint4 per k-step: [wave 4][ot][lane 64], the stem's f16 k-steps and the int8 ones alike
    // the ring, as in Geo: at 128 channels a k-step is 8-14 MFMAs and the ring as deep as the registers allow — the nine taps
    // unrolled, nine stages —; at 256 four stages, one per k-step of a tap.  Sixteen tiles: a k-step is 32 MFMAs of eight passes,
    // a thousand cycles, and six stages ask for a fragment three L2 round trips ahead; nine would spill
    static constexpr int PF = G == 2 ? (NT >= 16 ? 6 : 9) : 4;
    static constexpr int U = G == 2 ? 9 : 1;
    static_assert((U * G) % PF == 0 && (9 * G) % PF == 0, "ring stage of a k-step must be a compile-time constant");
    static_assert(C % 64 == 0 && LDS_BYTES <= 160 * 1024, "LDS budget");
    // byte offset within a plane's row pair of channel c: plane (c >= C/2), then the channel inside it
    __device__ static constexpr int chan_off(int c) { return c >= C / 2 ? PLANE + c - C / 2 : c; }
};

struct I8Dev {
    const h16 *x0;       // encoded input [batch*hw][ldx0] f16 (in.bits == nullptr)
    const uint4 *w;      // 9 * stem_chunks stem k-steps of f16 fragments, then 2*depth*9*C/64 k-steps of int8 fragments
    const float *bias;   // [1 + 2*depth][C]
    const float *mult;   // [1 + 2*depth][C]: 2^(e_in + f_oc) of layer l's output channels (row 0, the stem's, is not read)
    const float *qscale; // [2*depth]: 2^-e_s of site s (the stem's output, then every layer's but the last)
    const float *post_scale, *post_shift;
    h16 *y;              // tower output [batch*hw][ldy] f16
    int ldx0, ldy, batch, depth, h, w_, hw, nb;
    int stem_chunks;
    unsigned inv_w, inv_hw;  // ceil(65536 / w), ceil(65536 / hw): exact quotients for values < 512
    PackedBoards in;
    // HEADS == 2 (conv policy heads and the scalar head inside the launch): the policy head's Conv1x1 C->C + ReLU is one more
    // pass of C/32 f16 k-steps behind the tower's in `w`, its bias one more row of `bias`; then kz_conv_heads.hpp's members
    int hc, hs, pc, policy_len, zero_tail, extra;
    const float *sh_b0, *sh_w1t, *sh_b1, *sh_w2, *sh_b2, *p_b1, *pe_bc, *pe_wl, *pe_bl;
    const uint4 *small_w16;  // the two small convolutions as f16 fragments (tower_split_pack_small_weights16)
    union { float *scalars; unsigned char *tap_base; }; union { float *policy; size_t tap_site_bytes; };  // (a tap instance — no heads — keeps its buffer in the heads' two output words: kz_kernels.hpp, tap_put)
    int *nonfinite_flag;
    int epoch;
    DecodeDev dec;  // dec.move_offsets set: decode_output inside the launch
};

// clamp(rne(v * qs), -127, 127) of four values as the four bytes of a word, the first channel lowest
__device__ __forceinline__ int quant4(f32x4 v, float qs) {
    int r = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float q = fminf(fmaxf(__builtin_rintf(v[j] * qs), -127.0f), 127.0f);
        r |= ((int)q & 0xff) << (8 * j);
    }
    return r;
}

// HEADS: 0 = the tower alone, its output as f16 rows in global memory; 2 = + the conv policy heads (ConvPolicyHead,
// AtaxxConvPolicyHead), the scalar head and decode_output, as in the plain-f16 launch (kz_tower_pairs.hpp, HEADS == 2 without
// SPLIT), on values the tower holds as f16 already:
//   the last layer writes its f16 output in place into X (this lane's own slot) instead of to global memory;
//   the policy head's hidden layer, Conv1x1 C->C + ReLU, is one more pass of the weight ring — C/32 k-steps of
//     v_mfma_f32_16x16x32_f16 over X, the accumulators started from its bias row — into YH, an f16 image in X's layout at Q_OFF:
//     the int8 images are dead behind the layer loop's last barrier;
//   X is ONE plane in natural channel order (rows of 2 C + 16 bytes), so lane group kq's 16-byte piece of k-step ch — channels
//     8 ch + {0, C/2, C/4, 3C/4}[kq] + j, the packers' assignment — is at byte 2 * {0, C/2, C/4, 3C/4}[kq] + 16 ch of the row.  At
//     256 channels kq and kq + 1 are 256 B apart: the chess launch's conflict-free pattern.  At 128 channels they are 128 B
//     apart and two lane groups share banks (two-way conflicts): 4 NT + 8 ceil(NT / 4) such fragment reads per wave and launch
//     beside the tower's 36 depth NT conflict-free ones, accepted;
//   the two small convolutions are f16 MFMAs on X and YH (row tiles over the waves), the tail kz_conv_heads.hpp with its
//     scratch behind the launch's own LDS and X as the decode's staging.
// TAP: the tap instance of the tower alone (kz_kernels.hpp, tap_put; kz_model_int8_taps): behind each of the three epilogue
// stores the four q bytes go to the site's image tensor — one 4-byte store at the site's start — and the f16 quadruple stored
// beside them to the site's stream tensor, tap_site_bytes / 2 behind it (the place of a split pair's lo half); a mid site has
// an image only, the last site — the store to a.y — a stream only.  Rows of real boards only.
template <int C, int NT, int HEADS = 0, bool TAP = false>
__global__ __launch_bounds__(256, 1) void kz_tower_resident_i8(I8Dev a) {
    static_assert(HEADS == 0 || HEADS == 2, "0: the tower alone; 2: conv heads and decode inside");
    static_assert(!TAP || HEADS == 0, "the tap instance is the tower alone");
    using L = GeoI8<C, NT>;
    constexpr int PF = L::PF, RS = L::RS, XRS = L::XRS, OT = L::OT, G = L::G;
    constexpr int X8 = L::Q_OFF + L::X8, Y8 = L::Q_OFF + L::Y8, Z8 = L::Q_OFF + L::Z8;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int fr = lane & 15, kq = lane >> 4;
    const int board0 = blockIdx.x * a.nb;
    const int boards = min(a.nb, a.batch - board0);
    const int rows_valid = boards * a.hw;
    const int layers = 2 * a.depth;
    // of the ring: the stem's k-steps in front of them are read directly; the head pass follows the tower's
    const int total_ksteps = layers * 9 * G + (HEADS == 2 ? C / 32 : 0);

    // ---- weight stream: prime PF stages (stage s = k-step g % PF) ----
    const uint4 *wp_stem = a.w + wave * OT * 64 + lane;
    const int sc = a.stem_chunks;
    const uint4 *wp = wp_stem + (size_t)9 * sc * L::STEP;
    auto wload = [&](int gk, int ot) __attribute__((always_inline)) { return wp[(size_t)gk * L::STEP + ot * 64]; };
    uint4 wreg[PF][OT];
#pragma unroll
    for (int s = 0; s < PF; s++)
#pragma unroll
        for (int ot = 0; ot < OT; ot++) wreg[s][ot] = wload(s < total_ksteps ? s : total_ksteps - 1, ot);
    int g = 0;
    auto ring_take = [&](int stage, i32x4 (&af)[OT]) __attribute__((always_inline)) {
#pragma unroll
        for (int ot = 0; ot < OT; ot++) af[ot] = __builtin_bit_cast(i32x4, wreg[stage][ot]);
        const int gn = g + PF < total_ksteps ? g + PF : total_ksteps - 1;
#pragma unroll
        for (int ot = 0; ot < OT; ot++) wreg[stage][ot] = wload(gn, ot);
    };

    // ---- zero rows (both planes) and the stem input, staged as f16 in the Y8 image, which nothing else touches before the
    // first block's epilogue: rows of 64 B per chunk of 32 input planes, chunk k in plane k & 1 at (k >> 1) * 64 of a row of
    // 64 ceil(sc / 2) bytes (tower_i8_supported: such a row is no longer than a plane's) ----
    const int srow = 64 * ((sc + 1) >> 1), spieces = 8 * sc;
    auto stem_at = [&](int row, int chunk) __attribute__((always_inline)) {
        return Y8 + (chunk & 1) * L::PLANE + row * srow + (chunk >> 1) * 64;
    };
    for (int id = tid; id < 16 * RS / 16; id += 256) {
        *reinterpret_cast<uint4 *>(lds + Z8 + id * 16) = make_uint4(0, 0, 0, 0);
        *reinterpret_cast<uint4 *>(lds + Z8 + L::PLANE + id * 16) = make_uint4(0, 0, 0, 0);
    }
    for (int id = tid; id < L::ROWS * spieces; id += 256) {  // (row, 4-channel piece)
        const int row = id / spieces, c4 = id - row * spieces;
        h16x4 v = h16x4{};
        if (a.in.bits) {  // 4 channels of one square (kz_encode_dev.hpp)
            if (row < rows_valid) {
                const int b = (int)(((unsigned)row * a.inv_hw) >> 16), q = row - b * a.hw;
#pragma unroll
                for (int j = 0; j < 4; j++) v[j] = (h16)encoded_plane(a.in, board0 + b, c4 * 4 + j, q, a.hw);
            }
        } else if (row < rows_valid && c4 * 4 < a.ldx0) {
            v = *reinterpret_cast<const h16x4 *>(a.x0 + ((size_t)board0 * a.hw + row) * a.ldx0 + c4 * 4);
        }
        *reinterpret_cast<h16x4 *>(lds + stem_at(row, c4 >> 3) + (c4 & 7) * 8) = v;
    }

    // Validity of (tile row, tap) as bitmasks: bit nt of okmask[tap] says that for this lane's row of tile nt the tap
    // lands on the same board
    // (sixteen tiles: sixteen bits per tap, two taps to a register — taps 2 i and 2 i + 1 in the halves of okmask[i]; a reader
    // looks at bit nt < 16 of what ok_of returns and at nothing above it)
    constexpr int OKW = NT >= 16 ? 5 : 9;
    unsigned okmask[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        const int r = nt * 16 + fr;
        const int b = (int)(((unsigned)r * a.inv_hw) >> 16), q = r - b * a.hw;
        const unsigned valid = r < rows_valid;
        const int yy = (int)(((unsigned)q * a.inv_w) >> 16), xx = q - yy * a.w_;
        const unsigned ym[3] = {(unsigned)(yy >= 1), 1u, (unsigned)(yy <= a.h - 2)};
        const unsigned xm[3] = {(unsigned)(xx >= 1), 1u, (unsigned)(xx <= a.w_ - 2)};
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const unsigned bit = valid & ym[tap / 3] & xm[tap % 3];
            if constexpr (OKW == 9) okmask[tap] |= bit << nt;
            else okmask[tap >> 1] |= bit << (nt + 16 * (tap & 1));
        }
    }
    __syncthreads();
    auto ok_of = [&](int tap) __attribute__((always_inline)) {
        if constexpr (OKW == 9) {
            return tap == 0   ? okmask[0] : tap == 1 ? okmask[1] : tap == 2 ? okmask[2] : tap == 3 ? okmask[3]
                   : tap == 4 ? okmask[4] : tap == 5 ? okmask[5] : tap == 6 ? okmask[6] : tap == 7 ? okmask[7] : okmask[8];
        } else {
            const int i = tap >> 1;
            const unsigned pair = i == 0 ? okmask[0] : i == 1 ? okmask[1] : i == 2 ? okmask[2] : i == 3 ? okmask[3] : okmask[4];
            return pair >> (16 * (tap & 1));
        }
    };

    // per-channel tables of a layer — bias and 2^(e_in + f_oc) of this lane's channels — are fetched a layer ahead: a load that
    // is consumed right away would make the compiler wait for vmcnt(0) and drain the weight ring once per layer
    f32x4 bias_cur[OT], mult_cur[OT], bias_next[OT], mult_next[OT];
    auto fetch_tables = [&](int row) __attribute__((always_inline)) {
        const int l = row <= layers ? row : layers;
        const int lb = HEADS == 2 && row == layers + 1 ? row : l;  // (the head pass's bias row; `mult` has none for it)
#pragma unroll
        for (int ot = 0; ot < OT; ot++) {
            bias_next[ot] = *reinterpret_cast<const f32x4 *>(a.bias + lb * C + (wave * OT + ot) * 16 + kq * 4);
            mult_next[ot] = *reinterpret_cast<const f32x4 *>(a.mult + l * C + (wave * OT + ot) * 16 + kq * 4);
        }
    };
    // (sixteen tiles with the heads inside: ONE set — a layer's tables are fetched at the top of its own convolution, eighteen unrolled k-steps of
    // straight-line code in front of the epilogue that reads them, so the wait for them counts the ring's loads behind them and
    // drains nothing; sixteen registers the allocator needs there)
    constexpr bool ONE_TABLE = NT >= 16;
    static_assert(NT < 16 || HEADS == 2, "sixteen tiles exist with the heads inside only");
    auto &bias_use = *(ONE_TABLE ? &bias_next : &bias_cur);
    auto &mult_use = *(ONE_TABLE ? &mult_next : &mult_cur);
    auto take_tables = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int ot = 0; ot < OT; ot++) {
            bias_cur[ot] = bias_next[ot];
            mult_cur[ot] = mult_next[ot];
        }
    };

    // this lane's four channels of output tile ot, pixel row of tile nt: byte offsets within the f16 image and an int8 image
    const int oc0 = wave * OT * 16 + kq * 4;
    auto x_off = [&](int ot, int nt) __attribute__((always_inline)) { return (nt * 16 + fr) * XRS + (oc0 + ot * 16) * 2; };
    auto q_off = [&](int ot, int nt) __attribute__((always_inline)) { return (nt * 16 + fr) * RS + L::chan_off(oc0 + ot * 16); };
    // (TAP) this lane's four channels of a pixel row to the site's tensors: the image's q bytes, the stream's f16 values
    auto tap_image = [&](int site, int ot, int nt, int q) __attribute__((always_inline)) {
        tap_put(a, site, nt * 16 + fr < rows_valid, tap_elem(board0, a.hw, nt * 16 + fr, C, oc0 + ot * 16), q);
    };
    auto tap_stream = [&](int site, int ot, int nt, h16x4 xh) __attribute__((always_inline)) {
        tap_put(a, site, nt * 16 + fr < rows_valid, tap_elem(board0, a.hw, nt * 16 + fr, C, oc0 + ot * 16), xh, a.tap_site_bytes / 2);
    };
    auto tap_site = [&](int site, int ot, int nt, int q, h16x4 xh) __attribute__((always_inline)) {
        tap_image(site, ot, nt, q);
        tap_stream(site, ot, nt, xh);
    };

    // ---- stem in f16, exactly as the plain-f16 launch: 9 sc k-steps over the 32 sc (padded) input channels; conv + bias, no
    // activation (post_act.py:205).  Its epilogue writes X and X8 = quant(v, e_0) ----
    {
        f32x4 sacc[OT][NT];
        fetch_tables(0);
#pragma unroll
        for (int ot = 0; ot < OT; ot++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++) sacc[ot][nt] = bias_next[ot];
        if constexpr (!ONE_TABLE) fetch_tables(1);
#pragma nounroll
        for (int ks = 0; ks < 9 * sc; ks++) {
            const int tap = sc == 1 ? ks : ks / sc, chunk = ks - tap * sc;
            const int shift = (tap / 3 - 1) * a.w_ + (tap % 3 - 1);
            const unsigned ok = ok_of(tap);
            h16x8 ah[OT], bh[NT];
#pragma unroll
            for (int ot = 0; ot < OT; ot++) {
                const uint4 th = wp_stem[(size_t)ks * L::STEP + ot * 64];
                ah[ot] = *reinterpret_cast<const h16x8 *>(&th);
            }
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                const int off = stem_at(nt * 16 + fr + shift, chunk) + kq * 16;  // stem: natural k (channel = 32 chunk + 8 kq + j)
                const bool valid = (ok >> nt) & 1;
                bh[nt] = valid ? *reinterpret_cast<const h16x8 *>(lds + off) : h16x8{};
            }
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
#pragma unroll
                for (int ot = 0; ot < OT; ot++)
                    sacc[ot][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[ot], bh[nt], sacc[ot][nt], 0, 0, 0);
        }
        const float qs = a.qscale[0];
#pragma unroll
        for (int ot = 0; ot < OT; ot++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                const f32x4 v = sacc[ot][nt];
                *reinterpret_cast<h16x4 *>(lds + x_off(ot, nt)) = h16x4{(h16)v[0], (h16)v[1], (h16)v[2], (h16)v[3]};
                *reinterpret_cast<int *>(lds + X8 + q_off(ot, nt)) = quant4(v, qs);
                if constexpr (TAP) tap_site(0, ot, nt, quant4(v, qs), h16x4{(h16)v[0], (h16)v[1], (h16)v[2], (h16)v[3]});
            }
    }
    __syncthreads();

    // ---- convolution passes over the int8 images ----
    const int kq_off = L::PLANE * (kq & 1) + (C / 4) * (kq >> 1);
    const int frag_base = fr * RS + kq_off;
    // T[nt] = LDS address of this lane's fragment row (pixel shifted by the tap) or of a zero row with the same slot
    auto tap_rows = [&](int tap, int src, int (&T)[NT]) __attribute__((always_inline)) {
        const int shift = (tap / 3 - 1) * a.w_ + (tap % 3 - 1);
        const unsigned ok = ok_of(tap);
        const int shifted = src + frag_base + shift * RS;
        const int zrow = Z8 + ((fr + shift) & 15) * RS + kq_off;
#pragma unroll
        for (int nt = 0; nt < NT; nt++) T[nt] = ((ok >> nt) & 1) ? shifted + nt * 16 * RS : zrow;
    };
    i32x4 acc[OT][NT];
    // Sixteen tiles: the accumulators (128 registers), a double buffer of fragments (128), the ring (72) and two sets of row
    // addresses (32) leave the register file no room and the allocator spills.  There the fragments live in THREE half
    // buffers: k-step s holds its tiles in halves 2 s and 2 s + 1 (mod 3), the next step's first half is read into the free
    // one under the first half's MFMAs and its second half into the half those have consumed; and one set of row addresses
    // serves — the next tap's replace this tap's in its last k-step, behind their last use.  Same reads, same MFMAs in the
    // same order per accumulator: the sums are the same integers.
    constexpr bool HALVES = NT >= 16;
    auto conv_3x3 = [&](int src) __attribute__((always_inline)) {
      if constexpr (HALVES) {
        constexpr int H = NT / 2;
        static_assert(NT % 2 == 0 && (L::U * G) % 3 == 0 && L::U == 9, "the half buffers' roles repeat with the unrolled body, which is a whole convolution");
        int T[NT];
        i32x4 hb[3][H];
        tap_rows(0, src, T);
        auto rd = [&](int t, int extra) __attribute__((always_inline)) { return *reinterpret_cast<const i32x4 *>(lds + t + extra); };
#pragma unroll
        for (int nt = 0; nt < H; nt++) {
            hb[0][nt] = rd(T[nt], 0);
            hb[1][nt] = rd(T[H + nt], 0);
        }
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
#pragma unroll
            for (int ch = 0; ch < G; ch++) {
                const int s = tap * G + ch, stage = s % PF;
                const int b0 = (2 * s) % 3, b1 = (2 * s + 1) % 3, b2 = (2 * s + 2) % 3;
                if (ch == G - 1) tap_rows(tap + 1 < 9 ? tap + 1 : tap, src, T);
                const int extra = ch < G - 1 ? (ch + 1) * 16 : 0;
#pragma unroll
                for (int nt = 0; nt < H; nt++) hb[b2][nt] = rd(T[nt], extra);
                i32x4 af[OT];
                ring_take(stage, af);
#pragma unroll
                for (int nt = 0; nt < H; nt++)
#pragma unroll
                    for (int ot = 0; ot < OT; ot++)
                        acc[ot][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[ot], hb[b0][nt], acc[ot][nt], 0, 0, 0);
#pragma unroll
                for (int nt = 0; nt < H; nt++) hb[b0][nt] = rd(T[H + nt], extra);
#pragma unroll
                for (int nt = 0; nt < H; nt++)
#pragma unroll
                    for (int ot = 0; ot < OT; ot++)
                        acc[ot][H + nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[ot], hb[b1][nt], acc[ot][H + nt], 0, 0, 0);
                // the ring refills and the first half's reads each behind an MFMA of the first half; the second half's reads
                // behind the MFMAs that free their registers; then the remaining MFMAs back to back
                constexpr int HMF = OT * H;
                static_assert(OT + H <= HMF, "a half's MFMAs cover the ring refills and a half's reads");
#pragma unroll
                for (int i = 0; i < OT; i++) {
                    __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(SG_VMEM_READ, 1, 0);
                }
#pragma unroll
                for (int i = 0; i < H; i++) {
                    __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(SG_DS_READ, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(SG_MFMA, HMF - OT - H, 0);
#pragma unroll
                for (int i = 0; i < H; i++) {
                    __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(SG_DS_READ, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(SG_MFMA, HMF - H, 0);
                __builtin_amdgcn_sched_barrier(0);
                g++;
            }
        }
      } else {
        int T[NT], Tn[NT];
        i32x4 bf[2][NT];
        tap_rows(0, src, T);
        auto rd = [&](int t, int extra) __attribute__((always_inline)) { return *reinterpret_cast<const i32x4 *>(lds + t + extra); };
#pragma unroll
        for (int nt = 0; nt < NT; nt++) bf[0][nt] = rd(T[nt], 0);
#pragma nounroll
        for (int tb = 0; tb < 9; tb += L::U)
#pragma unroll
        for (int tu = 0; tu < L::U; tu++) {
            const int tap = tb + tu;
            tap_rows(tap + 1 < 9 ? tap + 1 : tap, src, Tn);
#pragma unroll
            for (int ch = 0; ch < G; ch++) {
                const int stage = (tu * G + ch) % PF, cur = (tu * G + ch) & 1, nxt = cur ^ 1;
#pragma unroll
                for (int nt = 0; nt < NT; nt++) bf[nxt][nt] = ch < G - 1 ? rd(T[nt], (ch + 1) * 16) : rd(Tn[nt], 0);
                i32x4 af[OT];
                ring_take(stage, af);
#pragma unroll
                for (int nt = 0; nt < NT; nt++)
#pragma unroll
                    for (int ot = 0; ot < OT; ot++)
                        acc[ot][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[ot], bf[cur][nt], acc[ot][nt], 0, 0, 0);
                // every memory instruction in the shadow of an MFMA: the ring refills, the fragment reads, then the
                // remaining MFMAs back to back
                constexpr int NMF = OT * NT, NVM = OT, NDS = NT;
                constexpr int PAIRED = NVM + NDS < NMF ? NVM + NDS : NMF;
#pragma unroll
                for (int i = 0; i < NVM; i++) {
                    if (i < PAIRED) __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(SG_VMEM_READ, 1, 0);
                }
#pragma unroll
                for (int i = 0; i < NDS; i++) {
                    if (NVM + i < PAIRED) __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(SG_DS_READ, 1, 0);
                }
                if constexpr (NMF > PAIRED) __builtin_amdgcn_sched_group_barrier(SG_MFMA, NMF - PAIRED, 0);
                __builtin_amdgcn_sched_barrier(0);
                g++;
            }
#pragma unroll
            for (int nt = 0; nt < NT; nt++) T[nt] = Tn[nt];
        }
      }
    };
    static_assert(G % 2 == 0, "the double buffer's parity is a tap's own: an even number of k-steps per tap");

    // ---- the 2*depth 3x3 convolutions ----
    for (int layer = 1; layer <= layers; layer++) {
        const bool is_b = (layer & 1) == 0;  // conv A: X8 -> Y8; conv B: Y8 -> X, X8 (+ residual)
        if constexpr (ONE_TABLE) {
            fetch_tables(layer);
        } else {
            take_tables();
            fetch_tables(layer + 1);
        }
#pragma unroll
        for (int ot = 0; ot < OT; ot++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++) acc[ot][nt] = i32x4{0, 0, 0, 0};
        conv_3x3(is_b ? Y8 : X8);
        const float qs = a.qscale[layer < layers ? layer : layers - 1];  // (the last layer's output is not quantised)
#pragma unroll
        for (int ot = 0; ot < OT; ot++) {
            f32x4 ps = f32x4{1.f, 1.f, 1.f, 1.f}, pt = f32x4{0.f, 0.f, 0.f, 0.f};
            if (layer == layers) {
                ps = *reinterpret_cast<const f32x4 *>(a.post_scale + oc0 + ot * 16);
                pt = *reinterpret_cast<const f32x4 *>(a.post_shift + oc0 + ot * 16);
            }
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    v[j] = (float)acc[ot][nt][j] * mult_use[ot][j] + bias_use[ot][j];
                    v[j] = v[j] > 0.0f ? v[j] : 0.0f;
                }
                if (!is_b) {
                    *reinterpret_cast<int *>(lds + Y8 + q_off(ot, nt)) = quant4(v, qs);
                    if constexpr (TAP) tap_image(layer, ot, nt, quant4(v, qs));
                    continue;
                }
                const h16x4 rx = *reinterpret_cast<const h16x4 *>(lds + x_off(ot, nt));
#pragma unroll
                for (int j = 0; j < 4; j++) v[j] += (float)rx[j];  // added in f32, AFTER the ReLU (post_act.py:227-228)
                if (layer != layers) {
                    *reinterpret_cast<h16x4 *>(lds + x_off(ot, nt)) = h16x4{(h16)v[0], (h16)v[1], (h16)v[2], (h16)v[3]};
                    *reinterpret_cast<int *>(lds + X8 + q_off(ot, nt)) = quant4(v, qs);
                    if constexpr (TAP) tap_site(layer, ot, nt, quant4(v, qs), h16x4{(h16)v[0], (h16)v[1], (h16)v[2], (h16)v[3]});
                } else {
                    // last layer: the final BN in f32 -> f16 rows of the tower output in global memory
                    v = v * ps + pt;
                    if constexpr (HEADS != 0) {  // the heads read the tower output from X (in place: this lane owns the slot)
                        *reinterpret_cast<h16x4 *>(lds + x_off(ot, nt)) = h16x4{(h16)v[0], (h16)v[1], (h16)v[2], (h16)v[3]};
                        continue;
                    }
                    const int r = nt * 16 + fr;
                    if (r < rows_valid)
                        *reinterpret_cast<h16x4 *>(a.y + ((size_t)board0 * a.hw + r) * a.ldy + oc0 + ot * 16) =
                            h16x4{(h16)v[0], (h16)v[1], (h16)v[2], (h16)v[3]};
                    if constexpr (TAP) tap_stream(layers, ot, nt, h16x4{(h16)v[0], (h16)v[1], (h16)v[2], (h16)v[3]});  // (the last site: what the launch hands on)
                }
            }
        }
        __syncthreads();
    }

    if constexpr (HEADS == 2) {
        // ---- conv policy heads (post_act.py:75-110) and scalar head (post_act.py:8-31) ----
        constexpr int GH = C / 32, YH = L::Q_OFF;
        static_assert(L::ROWS * XRS <= 2 * L::PLANE, "the hidden image fits the dead int8 region");
        static_assert((9 * G) % PF == 0, "the head pass starts at ring stage 0");
        const int kx_off = 2 * ((C / 2) * (kq & 1) + (C / 4) * (kq >> 1));
        // The policy head's hidden layer, Conv1x1 C->C + ReLU: one more pass of the weight ring over X into YH
        if constexpr (ONE_TABLE) fetch_tables(layers + 1);  // (read at once: the one drain of the ring per launch)
        else take_tables();
        f32x4 hacc[OT][NT];
#pragma unroll
        for (int ot = 0; ot < OT; ot++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++) hacc[ot][nt] = bias_use[ot];
#pragma unroll
        for (int ch = 0; ch < GH; ch++) {
            h16x8 bh[NT];
#pragma unroll
            for (int nt = 0; nt < NT; nt++) bh[nt] = *reinterpret_cast<const h16x8 *>(lds + (nt * 16 + fr) * XRS + kx_off + ch * 16);
            i32x4 af[OT];
            ring_take(ch % PF, af);
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
#pragma unroll
                for (int ot = 0; ot < OT; ot++)
                    hacc[ot][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, af[ot]), bh[nt], hacc[ot][nt], 0, 0, 0);
            g++;
        }
#pragma unroll
        for (int ot = 0; ot < OT; ot++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                f32x4 v = hacc[ot][nt];
#pragma unroll
                for (int j = 0; j < 4; j++) v[j] = v[j] > 0.0f ? v[j] : 0.0f;
                *reinterpret_cast<h16x4 *>(lds + YH + x_off(ot, nt)) = h16x4{(h16)v[0], (h16)v[1], (h16)v[2], (h16)v[3]};
            }
        __syncthreads();
        // The two small convolutions as f16 MFMAs straight on the two f16 images, row tiles split over the waves (the plain-f16
        // launch's provider on one-plane images); the tail's scratch is BEHIND the launch's own LDS (the launcher asks for it)
        constexpr int TW = (NT + 3) / 4;
        auto small_conv = [&](int which, auto emit) {
            const int img = which ? YH : 0;
            const uint4 *wfrag = a.small_w16 + which * (GH * 2 * 64);  // [GH][2][64]
            f32x4 sa[2][TW];
            int base[TW];
#pragma unroll
            for (int t = 0; t < TW; t++) {
                sa[0][t] = sa[1][t] = f32x4{0, 0, 0, 0};
                const int row = (wave + 4 * t) * 16 + fr;
                base[t] = img + (row < L::ROWS ? row : L::ROWS - 1) * XRS + kx_off;
            }
#pragma unroll
            for (int gs = 0; gs < GH; gs++) {
                const uint4 w0 = wfrag[(gs * 2 + 0) * 64 + lane], w1 = wfrag[(gs * 2 + 1) * 64 + lane];
                const h16x8 a0 = __builtin_bit_cast(h16x8, w0), a1 = __builtin_bit_cast(h16x8, w1);
#pragma unroll
                for (int t = 0; t < TW; t++) {
                    const h16x8 b = *reinterpret_cast<const h16x8 *>(lds + base[t] + gs * 16);
                    sa[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b, sa[0][t], 0, 0, 0);
                    sa[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b, sa[1][t], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < TW; t++) {
                const int row = (wave + 4 * t) * 16 + fr;
                if (wave + 4 * t < NT && row < rows_valid) {
#pragma unroll
                    for (int mt = 0; mt < 2; mt++)
#pragma unroll
                        for (int q = 0; q < 4; q++) emit(mt, q, row, sa[mt][t][q]);
                }
            }
        };
        conv_heads_tail<C, NT>(a, lds, L::LDS_BYTES, board0, boards, rows_valid, small_conv, 0, L::XIMG);
    }
}

template <int C, int NT, int HEADS = 0, bool TAP = false>
void launch(const I8Dev &d, int grid, hipStream_t stream) {
    static_assert(GeoI8<C, NT>::LDS_BYTES == i8_own_lds_bytes(C, NT), "the host's restatement of the LDS geometry");
    constexpr int LDS = GeoI8<C, NT>::LDS_BYTES + (HEADS == 2 ? i8_tail_scratch_bytes(C, NT) : 0);
    static_assert(LDS <= 160 * 1024, "LDS budget");
    allow_dynamic_lds<kz_tower_resident_i8<C, NT, HEADS, TAP>>(LDS);
    kz_tower_resident_i8<C, NT, HEADS, TAP><<<grid, 256, LDS, stream>>>(d);
}

// The instance of (channels, nt) among I8_ROWS, with the conv heads' tail if asked for: no such row = no launch (false).
// tap: the tap instance, which every plain row has and no other
template <size_t... I>
bool launch_row(std::index_sequence<I...>, int channels, int nt, bool conv_heads, bool tap, const I8Dev &d, int grid, hipStream_t stream) {
    return (... || [&] {
        constexpr I8Row R = I8_ROWS[I];
        if (R.c != channels || R.nt != nt) return false;
        if (!conv_heads) {
            if constexpr (R.plain) {
                if (tap) launch<R.c, R.nt, 0, true>(d, grid, stream);
                else launch<R.c, R.nt>(d, grid, stream);
            }
            return R.plain;
        }
        if (tap) return false;
        if constexpr (R.conv_heads) launch<R.c, R.nt, 2>(d, grid, stream);
        return R.conv_heads;
    }());
}

}  // namespace

// (the stem's input planes, in chunks of 32, are staged as f16 rows in the Y8 image: 64 B per pair of chunks and row must fit a
// plane's row of C / 2 + 16 B)
bool tower_i8_supported(int h, int w, int channels, int depth, int c_in) {
    const int sc = (c_in + 31) / 32;
    return depth >= 1 && c_in >= 1 && 64 * ((sc + 1) / 2) <= channels / 2 + 16 && h >= 2 && w >= 2 && w <= 32 &&
           i8_tiles_for(h * w, channels) != 0;
}

bool tower_i8_wide_supported(int h, int w, int channels, int max_batch, int heads_cap) {
    return i8_tiles_for(h * w, channels) != 0 && i8_wide_tiles_for(h * w, channels, max_batch, heads_cap) != 0;
}

int tower_i8_boards_per_workgroup(int h, int w, int channels, int wide_batch, int heads_cap) {
    const int nt = i8_tiles(h * w, channels, wide_batch, heads_cap);
    return nt ? nt * 16 / (h * w) : 0;
}

namespace {
bool i8_tail_fits(int nt, int policy_kind, int extra_moves, int pc, int h, int w, int channels, int hc, int hs) {
    if (!nt || !i8_has_row(channels, nt, true)) return false;
    return conv_heads_fit(nt, policy_kind, extra_moves, pc, h, w, channels, hc, hs, (size_t)i8_tail_scratch_bytes(channels, nt));
}
}  // namespace

// kz_conv_heads.hpp behind the narrow tiles: what decides whether the launch carries the heads at all
bool tower_i8_conv_heads_supported(int policy_kind, int extra_moves, int pc, int h, int w, int channels, int hc, int hs) {
    return i8_tail_fits(i8_tiles_for(h * w, channels), policy_kind, extra_moves, pc, h, w, channels, hc, hs);
}

// ... and behind the wide ones: the tile count of the widest wide level of this shape whose tail fits (at most four boards, its
// floats within the scratch left behind that level's own LDS), 0 if none does.  A level is asked at a batch that selects it.
int tower_i8_conv_heads_wide_cap(int policy_kind, int extra_moves, int pc, int h, int w, int channels, int hc, int hs) {
    for (int cap = 16; cap >= 8; cap--) {
        const int nt = i8_wide_tiles_for(h * w, channels, 1 << 20, cap);
        if (nt != cap) continue;  // (no level of exactly `cap` tiles)
        if (i8_tail_fits(nt, policy_kind, extra_moves, pc, h, w, channels, hc, hs)) return nt;
    }
    return 0;
}

size_t tower_i8_layer_bytes(int channels) { return (size_t)9 * channels * channels; }

// [C out][C in][9] int8 (OIHW, quantised) -> the 9 * C/64 k-steps of a block convolution, [tap][chunk] of
// [wave 4][ot C/64][lane 64][16] int8: byte j of lane (fr, kq) of (wave, ot) is
// wq[oc = 16*(wave*C/64 + ot) + fr][channel = {0, C/2, C/4, 3C/4}[kq] + 16*chunk + j][tap] — the A fragment of
// v_mfma_i32_16x16x64_i8 with the k order of the kernel's LDS reads
void tower_i8_pack_weights(const int8_t *wq, int channels, int8_t *dst) {
    const int C = channels, ot_n = C / 64, g_n = C / 64;
    const int kq_base[4] = {0, C / 2, C / 4, 3 * C / 4};
    for (int tap = 0; tap < 9; tap++)
        for (int chunk = 0; chunk < g_n; chunk++) {
            int8_t *step = dst + ((size_t)tap * g_n + chunk) * C * 64;
            for (int wave = 0; wave < 4; wave++)
                for (int ot = 0; ot < ot_n; ot++)
                    for (int lane = 0; lane < 64; lane++)
                        for (int j = 0; j < 16; j++) {
                            const int oc = 16 * (wave * ot_n + ot) + (lane & 15);
                            const int ch = kq_base[lane >> 4] + 16 * chunk + j;
                            step[(((size_t)wave * ot_n + ot) * 64 + lane) * 16 + j] = wq[((size_t)oc * C + ch) * 9 + tap];
                        }
        }
}

bool launch_tower_i8(const Tower32Args &t, const float *mult, const float *qscale, hipStream_t stream, int *nt_out) {
    I8Dev d{};
    d.in = t.in;
    d.x0 = reinterpret_cast<const h16 *>(t.x0);  // (f16 tensors behind the float pointers, as for launch_tower_pairs)
    d.ldx0 = t.ldx0;
    d.w = static_cast<const uint4 *>(t.weights);
    d.bias = t.bias;
    d.mult = mult;
    d.qscale = qscale;
    d.post_scale = t.post_scale;
    d.post_shift = t.post_shift;
    d.y = reinterpret_cast<h16 *>(t.y);
    d.ldy = t.ldy;
    d.batch = t.batch;
    d.depth = t.depth;
    d.h = t.h;
    d.w_ = t.w;
    d.hw = t.h * t.w;
    d.stem_chunks = (t.c_in + 31) / 32;
    // (wide_cap != 0: the heads are inside.  A tap launch runs the level of the batch whose geometry is tapped, on however few boards)
    const int nt = i8_tiles(d.hw, t.channels, t.wide ? (t.taps.base && t.tap_wide_batch ? t.tap_wide_batch : t.batch) : 0, t.wide_cap);
    if (nt_out) *nt_out = nt;
    if (!nt) return false;
    d.nb = nt * 16 / d.hw;
    d.inv_w = (65536u + (unsigned)t.w - 1) / (unsigned)t.w;
    d.inv_hw = (65536u + (unsigned)d.hw - 1) / (unsigned)d.hw;
    const int grid = (t.batch + d.nb - 1) / d.nb;
    const Tower32Args::Heads &hd = t.heads;
    if (hd.kind == Tower32Args::Heads::Kind::attention) return false;  // (no attention heads in this launch)
    const bool conv_heads = hd.kind == Tower32Args::Heads::Kind::conv;  // "...+heads" (the engine asked tower_i8_conv_heads_supported)
    if (conv_heads) {
        d.hc = hd.hc; d.hs = hd.hs; d.pc = hd.pc; d.policy_len = hd.policy_len; d.zero_tail = hd.zero_tail; d.extra = hd.extra;
        d.sh_b0 = hd.sh_b0; d.sh_w1t = hd.sh_w1t; d.sh_b1 = hd.sh_b1; d.sh_w2 = hd.sh_w2; d.sh_b2 = hd.sh_b2;
        d.p_b1 = hd.p_b1; d.pe_bc = hd.pe_bc; d.pe_wl = hd.pe_wl; d.pe_bl = hd.pe_bl;
        d.small_w16 = reinterpret_cast<const uint4 *>(hd.small_w);
        d.scalars = hd.scalars; d.policy = hd.policy;
        d.nonfinite_flag = hd.nonfinite_flag; d.epoch = hd.epoch;
        d.dec = decode_dev(hd.decode, true, hd.policy_len);
    }
    if (t.taps.base) {  // (in the words of the heads' two outputs: a tap launch has no heads)
        if (conv_heads) return false;
        d.tap_base = t.taps.base;
        d.tap_site_bytes = t.taps.site_bytes;
    }
    return launch_row(std::make_index_sequence<std::size(I8_ROWS)>{}, t.channels, nt, conv_heads, t.taps.base != nullptr, d, grid, stream);
}

}  // namespace kz
