// Micro-benchmark: the matrix cores' power ceiling (= the clock the chip sustains) per ISSUE ORDER of the
// f16 tower's super-step, with the kernel's operand traffic instead of mfma_power.hip's ten loop-invariant fragments:
//  * 8 B fragments (line fragments), double buffered, refilled once per super-step with ds_read_b128 from an LDS image
//    of 16 super-steps that is written once: post-ReLU N(0,1) data (half zeros), or dense N(0,1) data (conv A's input is
//    post-ReLU, a residual stream is not);
//  * 12 A fragments (weights) per super-step out of a register ring of 4 k-steps, refilled with global_load_dwordx4
//    from a 72-k-step weight stream (1.15 MB, one layer's) that stays in L2, all workgroups reading the same one;
//  * 4 x 8 accumulator tiles and the tile ranges 1..7 / 0..7 / 0..6 of the three tap rows: 88 MFMAs per super-step;
//  * the kernel's issue pipeline: the 4 refills behind the first four MFMAs of a k-step, the 8 fragment reads behind
//    the next eight of the super-step's first k-step;
//  * one wave per SIMD (256 workgroups of 4 waves), launches of about 150 ms.
// Orders:  a  nt outer, mt ascending (the kernel's before kz_tower_mfma_order.hpp)
//          b  boustrophedon in mt, no seam carried (dy = 0 starts at the high end)
//          c  boustrophedon in mt, B register carried over the dy seam where the range has it (kz_tower_mfma_order.hpp)
//          d  mt outer: the B fragment is held and the weight fragment changes with every MFMA (control)
// Prints wall-clock TFLOP/s per launch; `--rounds R` interleaves the orders R times so that the run-to-run spread of
// one order is seen on the same box in the same minute.  `--quick` is one round of two launches (for a counter pass).
// Build: hipcc --offload-arch=gfx950 -O3 -o tools/micro/mfma_order tools/micro/mfma_order.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>
#include "../../kzero_amd/csrc/kz_tower_mfma_order.hpp"

typedef _Float16 h16;
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MT = 8, NT = kz_mfma_order::NT, PF = 4, SLOTS = 16, SUPER = 24, KSTEPS = 3 * SUPER;
constexpr int SLOT_BYTES = MT * 64 * 16, LDS_BYTES = SLOTS * SLOT_BYTES, KSTEP_BYTES = 4 * NT * 64 * 16;
constexpr int SG_MFMA = 0x8, SG_VMEM_READ = 0x20, SG_DS_READ = 0x100;
static_assert(KSTEPS % PF == 0 && SUPER % 2 == 0, "ring stage and fragment buffer are the same at every layer's start");

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

enum { ORDER_A, ORDER_B, ORDER_C, ORDER_D };

// (nt, mt) of MFMA j of k-step i
template <int ORDER>
constexpr kz_mfma_order::Pos order_at(int i, int j) {
    constexpr kz_mfma_order::Rows R = kz_mfma_order::line_rows(MT);
    const int lo = R.lo[i], hi = R.hi[i], n = hi - lo;
    if (ORDER == ORDER_A) return {j / n, lo + j % n};
    if (ORDER == ORDER_B) return kz_mfma_order::boustrophedon(lo, hi, i == 1, j);
    if (ORDER == ORDER_C) return kz_mfma_order::at(R, i, j);
    return {j % NT, lo + j / NT};
}

// DENSE only names the instance (the counter pass tells the launches apart by kernel name); the data come from xsrc
template <int ORDER, bool DENSE>
__global__ __launch_bounds__(256, 1) void k_order(const unsigned char *wsrc, const uint4 *xsrc, int layers, float *sink) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int id = tid; id < LDS_BYTES / 16; id += 256) *reinterpret_cast<uint4 *>(lds + id * 16) = xsrc[id];
    __syncthreads();

    typedef const __attribute__((address_space(1))) unsigned char *gptr;
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const unsigned wlane = lane * 16;
    const gptr w0 = (gptr)wsrc + wave * 4096;
    auto wload = [&](gptr k, int nt) __attribute__((always_inline)) {
        return __builtin_bit_cast(uint4, *reinterpret_cast<const __attribute__((address_space(1))) u32x4 *>(k + wlane + nt * 1024));
    };
    uint4 wreg[PF][NT];
#pragma unroll
    for (int s = 0; s < PF; s++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) wreg[s][nt] = wload(w0 + s * KSTEP_BYTES, nt);

    f32x4 acc[NT][MT], total = f32x4{0, 0, 0, 0};
    h16x8 bf[2][MT];
    const int frag = lane * 16;
#pragma unroll
    for (int mt = 0; mt < MT; mt++) bf[0][mt] = *reinterpret_cast<const h16x8 *>(lds + frag + mt * 1024);

    // one trip = one layer: 24 super-steps in one basic block, as the kernel's.  The accumulators live for one layer:
    // their first MFMA takes `total` as C, and the layer's "epilogue" folds them into it.
#pragma unroll 1
    for (int layer = 0; layer < layers; layer++) {
        // k-steps PF.. of the stream (its first PF are in the ring: at the first layer from above, later the PF k-steps
        // of padding behind the stream, which the previous layer's last refills fetched)
        gptr wk = w0 + PF * KSTEP_BYTES;
        asm("" : "+s"(wk));
        static_for<0, SUPER>([&](auto ss_tag) __attribute__((always_inline)) {
            constexpr int ss = decltype(ss_tag)::value, cur = ss & 1, nxt = cur ^ 1;
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
                bf[nxt][mt] = *reinterpret_cast<const h16x8 *>(lds + frag + ((ss + 1) % SLOTS) * SLOT_BYTES + mt * 1024);
            static_for<0, 3>([&](auto i_tag) __attribute__((always_inline)) {
                constexpr int i = decltype(i_tag)::value, dy = i - 1, stage = (ss * 3 + i) & (PF - 1);
                constexpr int n = kz_mfma_order::count(kz_mfma_order::line_rows(MT), i);
                h16x8 af[NT];
#pragma unroll
                for (int nt = 0; nt < NT; nt++) af[nt] = *reinterpret_cast<const h16x8 *>(&wreg[stage][nt]);
#pragma unroll
                for (int nt = 0; nt < NT; nt++) wreg[stage][nt] = wload(wk, nt);
                wk += KSTEP_BYTES;
                asm("" : "+s"(wk));
                static_for<0, n>([&](auto j_tag) __attribute__((always_inline)) {
                    constexpr kz_mfma_order::Pos p = order_at<ORDER>(i, decltype(j_tag)::value);
                    constexpr bool opens = ss == 0 && (p.mt == 0 ? i == 1 : i == 0);  // the accumulator's first MFMA
                    acc[p.nt][p.mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[p.nt], bf[cur][p.mt + dy], opens ? total : acc[p.nt][p.mt], 0, 0, 0);
                });
#pragma unroll
                for (int j = 0; j < NT; j++) {
                    __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(SG_VMEM_READ, 1, 0);
                }
                constexpr int nr = i == 0 ? MT : 0;
#pragma unroll
                for (int j = 0; j < nr; j++) {
                    __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(SG_DS_READ, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(SG_MFMA, n - nr - NT, 0);
                __builtin_amdgcn_sched_barrier(0);
            });
        });
        f32x4 fold = f32x4{0, 0, 0, 0};
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int mt = 0; mt < MT; mt++) fold += acc[nt][mt];
        total = fold * 1e-3f;  // (stays finite over any number of layers)
    }
    float s = total[0] + total[1] + total[2] + total[3];
#pragma unroll
    for (int st = 0; st < PF; st++) s += __builtin_bit_cast(float, wreg[st][0].x);
    if (s == 123.456f) sink[tid] = s;
}

static float gauss() {
    const float u = (rand() + 1.0f) / ((float)RAND_MAX + 2.0f), v = (rand() + 1.0f) / ((float)RAND_MAX + 2.0f);
    return sqrtf(-2 * logf(u)) * cosf(6.2831853f * v);
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

struct Bufs {
    unsigned char *w;
    uint4 *x[2];  // post-ReLU, dense
    float *sink;
};

// `launches` timed launches behind `warm` untimed ones; returns the median TFLOP/s and prints every launch
template <int ORDER, bool DENSE>
static double run(const char *name, const Bufs &b, int iters, int warm, int launches) {
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_order<ORDER, DENSE>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::vector<double> tf;
    const double flop = 256.0 * 4 * iters * SUPER * 88 * 16384;
    for (int rep = 0; rep < warm + launches; rep++) {
        float ms = 0;
        CHECK(hipEventRecord(e0, 0));
        k_order<ORDER, DENSE><<<256, 256, LDS_BYTES>>>(b.w, b.x[DENSE], iters, b.sink);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipDeviceSynchronize());
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (rep >= warm) tf.push_back(flop / (ms * 1e-3) / 1e12);
    }
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
    printf("%-58s", name);
    for (double t : tf) printf(" %6.1f", t);
    std::sort(tf.begin(), tf.end());
    const double med = tf[tf.size() / 2];
    printf("  median %6.1f TFLOP/s (%.3f of 2500)\n", med, med / 2500);
    fflush(stdout);
    return med;
}

int main(int argc, char **argv) {
    int rounds = 3, warm = 3, launches = 5, iters = 6700;  // layers per launch: about 150 ms
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--quick")) { rounds = 1; warm = 1; launches = 2; }
        else if (!strcmp(argv[i], "--rounds") && i + 1 < argc) rounds = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--iters") && i + 1 < argc) iters = atoi(argv[++i]);
        else { fprintf(stderr, "usage: mfma_order [--quick] [--rounds R] [--iters N]\n"); return 2; }
    }
    const size_t nw = (size_t)(KSTEPS + PF) * KSTEP_BYTES / 2, nx = LDS_BYTES / 2;
    std::vector<h16> hw(nw), hx(nx), hd(nx);
    srand(1);
    for (auto &v : hw) v = (h16)(0.03f * gauss());
    for (auto &v : hx) { float g = gauss(); v = (h16)(g > 0 ? g : 0.0f); }
    for (auto &v : hd) v = (h16)gauss();
    Bufs b;
    CHECK(hipMalloc((void **)&b.w, nw * 2));
    CHECK(hipMalloc((void **)&b.x[0], nx * 2));
    CHECK(hipMalloc((void **)&b.x[1], nx * 2));
    CHECK(hipMalloc((void **)&b.sink, 4096));
    CHECK(hipMemcpy(b.w, hw.data(), nw * 2, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(b.x[0], hx.data(), nx * 2, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(b.x[1], hd.data(), nx * 2, hipMemcpyHostToDevice));

    static const char *names[8] = {
        "a  nt outer, mt ascending            post-ReLU B", "b  boustrophedon, no seam carried    post-ReLU B",
        "c  boustrophedon, B carried at seam  post-ReLU B", "d  mt outer (B held, A changes)      post-ReLU B",
        "a  nt outer, mt ascending            dense B",     "b  boustrophedon, no seam carried    dense B",
        "c  boustrophedon, B carried at seam  dense B",     "d  mt outer (B held, A changes)      dense B"};
    std::vector<std::vector<double>> med(8);
    for (int r = 0; r < rounds; r++) {
        printf("round %d\n", r);
        med[0].push_back(run<ORDER_A, false>(names[0], b, iters, warm, launches));
        med[1].push_back(run<ORDER_B, false>(names[1], b, iters, warm, launches));
        med[2].push_back(run<ORDER_C, false>(names[2], b, iters, warm, launches));
        med[3].push_back(run<ORDER_D, false>(names[3], b, iters, warm, launches));
        med[4].push_back(run<ORDER_A, true>(names[4], b, iters, warm, launches));
        med[5].push_back(run<ORDER_B, true>(names[5], b, iters, warm, launches));
        med[6].push_back(run<ORDER_C, true>(names[6], b, iters, warm, launches));
        med[7].push_back(run<ORDER_D, true>(names[7], b, iters, warm, launches));
    }
    printf("per order over %d rounds: min / median / max of the rounds' medians, spread = (max - min) / median, gain over a\n", rounds);
    for (int v = 0; v < 8; v++) {
        std::vector<double> m = med[v], a = med[v & 4];
        std::sort(m.begin(), m.end());
        std::sort(a.begin(), a.end());
        const double mid = m[m.size() / 2], amid = a[a.size() / 2];
        printf("%-58s %6.1f / %6.1f / %6.1f  spread %5.2f %%  vs a %+5.2f %%\n", names[v], m.front(), mid, m.back(), 100 * (m.back() - m.front()) / mid, 100 * (mid / amid - 1));
    }
    return 0;
}
