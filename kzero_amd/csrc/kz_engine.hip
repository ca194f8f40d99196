// kz_engine.hip — the executor behind the C ABI of include/kz_hip.h.
//
// One kz_engine = one `CudaNetwork` of the reference (rust/kz-core/src/network/cudnn.rs:18-88): a private HIP stream,
// private activation buffers sized for max_batch, pinned staging for the host-pointer entry points, and a shared,
// reference-counted copy of the device weights per (model, device, dtype).
// Forward schedule per batch: encode (F0) -> tower (one board-resident launch, or stem + 2*depth fused conv launches
// on the generic path) -> ScalarHead -> policy head.  Only `batch` rows are ever touched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/kz_hip.h"
#include "kz_kernels.hpp"
#include "kz_model.hpp"

namespace {

#include "kz_engine_util.hpp"     // g_err, fail, guarded, HIP_TRY
#include "kz_plan.hpp"            // Tower, PathPlan, plan_path: which kernels run a network
#include "kz_device_weights.hpp"  // DevConv, DeviceWeights::build(model, spec), the cache by WeightsKey

#include "kz_engine_state.hpp"    // Prof, kz_model, effective_model, struct kz_engine: streams, slots, staging (closes the namespace itself)
#include "kz_engine_forward.hpp"  // kz_engine::run_tower / run_heads / forward_*: the launches of a forward pass

// The experiment build's switches (experiments/build.sh; the product reads none of them): the measured-and-rejected kernel
// organisations, applied to the plan after plan_path.  Their hooks stay where they act: the tower4 / board_conv2 launches
// (kz_engine_forward.hpp), the board_conv2 packing (kz_device_weights.hpp) and the graph replay (kz_engine_state.hpp).
static void experiment_switches(const Model &m, int dtype, int cin_p, PathPlan &p) {
#ifdef KZ_EXPERIMENTS
    const auto env_int = [](const char *name) { return getenv(name) ? atoi(getenv(name)) : 0; };
    if (env_on("KZ_NO_TOWER_F16") && p.tower == Tower::resident_f16) {  // (chess f16 through the generic one-launch f16 tower)
        p.tower = kz::tower_split_supported(m.h, m.w, m.channels, m.depth, m.c_in, false) ? Tower::resident_f16g : Tower::conv_igemm;
        p.heads = p.wide = false;
    }
    p.nb4 = p.tower == Tower::resident_f16 && env_int("KZ_TOWER_NB") == 4 && cin_p == 32;
    if (p.nb4) p.heads = false;  // (the four-board launch has no fused heads yet)
    p.tower_prev = p.tower == Tower::resident_f16 && !p.nb4 && env_on("KZ_TOWER_PREV");
    p.t32_dense3 = p.tower == Tower::resident_f32 && env_int("KZ_T32_BOARDS") == 3 &&
                   kz::tower32_dense3_supported((int)m.policy_kind, m.policy_extra_moves, m.policy_conv_channels, m.h, m.w, m.channels,
                                                m.sh_conv.cout, m.sh_fc0.out, p.heads);
    p.att_heads = !p.heads && att_heads_one_launch(m, dtype);
    // (the opt-in board-conv organisation has its own weight packing)
    p.conv2 = env_on("KZ_BOARD_CONV2") && p.tower == Tower::board_conv_f16 &&
              kz::board_conv2_supported(dtype, m.h, m.w, m.channels, m.channels);
    p.graph = env_on("KZ_HIP_GRAPH") && !p.heads;
    p.no_zero_copy = env_on("KZ_NO_ZERO_COPY");  // (the staged-copy variant of the "+heads" launches, for A/B timing)
#endif
}

// Workgroups and boards per workgroup of the tower launch of `batch` boards under a plan — pure host logic over the kernels'
// own rules, so what kz_engine_launch_geometry and kz_model_launch_geometry report is what the launchers launch.  m: the
// network the kernels run (effective_model), dtype: the engine's arithmetic (f32 or f16) behind the dtype it was asked for.
static void launch_geometry_of(const Model &m, const PathPlan &p, int dtype, int batch, int *workgroups, int *boards_per_workgroup) {
    const int cin_p = round_up(m.c_in, 32), cp = round_up(m.channels, 32);
    int per = 0, wgs = 0;
    switch (p.tower) {
        case Tower::dense_net:
        case Tower::att_valu: per = 1; break;  // a workgroup is a board
        case Tower::att_mfma: per = kz::att_tower16_boards_per_workgroup(m.channels, m.att_dff, batch, dtype == KZ_DTYPE_F32); break;
        case Tower::resident_f16: per = cin_p > 32 ? 2 : p.tower_nb; break;
        case Tower::resident_f32: per = kz::tower32_boards_per_workgroup(m.h, m.w, m.channels); break;
        case Tower::resident_split16:
        case Tower::resident_f16g:  // (per launch: the widest level this batch fills the chip with)
        case Tower::resident_bf16g:
            per = kz::tower_split_boards_per_workgroup(m.h, m.w, m.channels, split_arithmetic(p), p.wide ? batch : 0);
            break;
        case Tower::resident_i8: per = kz::tower_i8_boards_per_workgroup(m.h, m.w, m.channels, p.wide ? batch : 0, p.wide_cap); break;
        case Tower::board_conv_f16:
        case Tower::board_conv_split16: wgs = kz::board_conv_workgroups(batch, m.h, m.w, m.channels); break;
        case Tower::board_conv_i8: wgs = kz::board_conv_workgroups(batch, m.h, m.w, kz::board_conv_i8_channels(m.channels)); break;
        case Tower::conv_igemm: wgs = kz::conv_workgroups(dtype, batch * m.h * m.w, cp); break;
    }
#ifdef KZ_EXPERIMENTS
    if (p.nb4) per = 4;
    if (p.t32_dense3) per = 3;
    if (p.conv2) wgs = kz::board_conv2_workgroups(batch, m.channels);
#endif
    if (per) wgs = (batch + per - 1) / per;
    *workgroups = wgs;
    *boards_per_workgroup = per;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

#define KZ_API __attribute__((visibility("default")))

KZ_API const char *kz_last_error(void) { return g_err.c_str(); }

KZ_API int kz_device_count(int *count) {
    return guarded("kz_device_count", [&]() -> int {
        if (!count) return fail("kz_device_count: null argument");
#ifdef KZ_EXPERIMENTS  // (tests/test_abi.py: the guard itself, on the experiment build only — the product reads no such switch)
        if (const char *t = getenv("KZ_TEST_THROW")) {
            if (t[0] == '1') throw std::length_error("vector::_M_default_append (KZ_TEST_THROW)");
            if (t[0] == '2') throw std::bad_alloc();
            if (t[0] == '3') throw 42;
        }
#endif
        HIP_TRY(hipGetDeviceCount(count));
        return 0;
    });
}

KZ_API int kz_device_pci_bus_id(int device, char *buf, size_t len) {
    return guarded("kz_device_pci_bus_id", [&]() -> int {
        if (!buf || len < 16) return fail("kz_device_pci_bus_id: buffer of at least 16 bytes needed");
        HIP_TRY(hipDeviceGetPCIBusId(buf, (int)len, device));
        return 0;
    });
}

KZ_API int kz_model_load_onnx_memory(const void *blob, size_t len, int input_scalar_channels, kz_model **out) {
    return guarded("kz_model_load_onnx_memory", [&]() -> int {
        if (!blob || !out) return fail("kz_model_load_onnx: null argument");
        std::string err;
        Model *m = kz::parse_onnx(blob, len, input_scalar_channels, err);
        if (!m) return fail("kz_model_load_onnx: " + err);
        *out = new kz_model(std::shared_ptr<Model>(m));
        return 0;
    });
}

KZ_API int kz_model_load_memory(const void *blob, size_t len, kz_model **out) {
    return guarded("kz_model_load_memory", [&]() -> int {
        if (!blob || !out) return fail("kz_model_load_memory: null argument");
        if (kz::looks_like_onnx(blob, len)) return kz_model_load_onnx_memory(blob, len, -1, out);
        std::string err;
        Model *m = kz::parse_model(blob, len, err);
        if (!m) return fail("kz_model_load: " + err);
        *out = new kz_model(std::shared_ptr<Model>(m));
        return 0;
    });
}

static int read_whole_file(const char *path, std::vector<uint8_t> &buf) {
    FILE *f = fopen(path, "rb");
    if (!f) return fail(std::string("kz_model_load: cannot open '") + path + "'");
    uint8_t tmp[1 << 16];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
    fclose(f);
    return 0;
}

KZ_API int kz_model_load(const char *path, kz_model **out) {
    return guarded("kz_model_load", [&]() -> int {
        if (!path || !out) return fail("kz_model_load: null argument");
        std::vector<uint8_t> buf;
        if (read_whole_file(path, buf)) return 1;
        return kz_model_load_memory(buf.data(), buf.size(), out);
    });
}

KZ_API int kz_model_load_onnx(const char *path, int input_scalar_channels, kz_model **out) {
    return guarded("kz_model_load_onnx", [&]() -> int {
        if (!path || !out) return fail("kz_model_load_onnx: null argument");
        std::vector<uint8_t> buf;
        if (read_whole_file(path, buf)) return 1;
        return kz_model_load_onnx_memory(buf.data(), buf.size(), input_scalar_channels, out);
    });
}

KZ_API void kz_model_free(kz_model *model) {
    try {
        delete model;
    } catch (...) {
    }
}

KZ_API int kz_model_get_info(const kz_model *model, kz_model_info *out) {
    return guarded("kz_model_get_info", [&]() -> int {
        if (!model || !out) return fail("kz_model_get_info: null argument");
        const Model &m = *model->m;
        out->input_channels = m.c_in;
        out->board_h = m.h;
        out->board_w = m.w;
        out->input_scalar_channels = m.n_scalar;
        out->input_bool_channels = m.n_bool;
        out->policy_len = m.policy_len;
        out->tower_depth = m.depth;
        out->tower_channels = m.channels;
        out->policy_kind = (int)m.policy_kind;
        out->bits_bytes = m.n_bool < 0 ? -1 : (int)bits_bytes(m);
        out->param_count = m.param_count;
        out->flops_per_eval = m.flops_per_eval;
        return 0;
    });
}

KZ_API void kz_engine_destroy(kz_engine *e) {
    if (!e) return;
    kz_engine_destroy(e->fallback);  // (the range fallback's sibling engine)
    if (e->audit) {  // (the audit's)
        kz_engine_destroy(e->audit->sibling);
        delete e->audit;
    }
    (void)hipSetDevice(e->device);
    for (auto st : e->slot_stream)
        if (st) (void)hipStreamSynchronize(st);
    e->prof.destroy();
#ifdef KZ_EXPERIMENTS
    for (auto &g : e->graphs) (void)hipGraphExecDestroy(g.exec);
#endif
    for (auto &s : e->slots)
        if (s.done) (void)hipEventDestroy(s.done);
    for (void *p : e->allocs) (void)hipFree(p);
    for (void *p : e->pinned) (void)hipHostFree(p);
    for (int i = 0; i < KZ_ENGINE_SLOTS; i++)
        if (e->slot_stream[i] && (i < 2 || e->slot_stream[i] != e->slot_stream[i & 1])) (void)hipStreamDestroy(e->slot_stream[i]);
    e->wts.reset();
    delete e;
}

static bool known_dtype(int dtype) {
    return dtype == KZ_DTYPE_F32 || dtype == KZ_DTYPE_F16 || dtype == KZ_DTYPE_F32_SPLIT16 || dtype == KZ_DTYPE_BF16 || int8_dtype(dtype);
}

// kz_engine_create; profile: the range profile's internal engine — exact f32, no environment switch read, whatever plan_path
// would choose.  per_layer (kz_model_range_profile): the per-layer implicit GEMM, every stash site a range measurement;
// resident (kz_model_range_profile_fast where tower32_supported holds): the one-launch f32 tower without heads, whose
// PROFILE instance measures in its epilogues — the same weight stream as an ordinary exact-f32 engine's (weights_spec).
// per_layer_hist, resident_hist (kz_model_range_histogram, _fast): the same two engines counting binades instead of taking maxima
// taps (kz_model_tower_taps, kz_model_error_profile): the engine kz_engine_create would make for (max_batch, dtype) — the
// effective model, plan_path with the environment switches — but never with the heads inside the launch, and with a tap buffer
// for tap_boards boards, which makes run_tower launch the tap instance.  taps_reference: the same on the one-launch exact-f32
// tower whatever plan_path says (no switch read), the error profile's reference where that kernel takes the shape;
// per_layer_deviation: its reference elsewhere, the range profile's per-layer engine whose stash sites are compared on the device
enum class Profile { none, per_layer, resident, per_layer_hist, resident_hist, taps, taps_reference, per_layer_deviation };
static bool profile_per_layer(Profile p) { return p == Profile::per_layer || p == Profile::per_layer_hist || p == Profile::per_layer_deviation; }
static bool profile_hist(Profile p) { return p == Profile::per_layer_hist || p == Profile::resident_hist; }
static bool profile_taps(Profile p) { return p == Profile::taps || p == Profile::taps_reference; }
static int create_engine(const kz_model *model, int device, int max_batch, int dtype, Profile profile, kz_engine **out, int tap_boards = 0) {
    {
        if (!model || !out) return fail("kz_engine_create: null argument");
        if (max_batch <= 0) return fail("kz_engine_create: max_batch must be positive");
        // every tensor of an engine is addressed with 32-bit byte offsets (buffer descriptors, int row indices): max_batch times
        // its bytes per board must stay below 2 GiB.  The largest one — an activation row set in f32, or the policy rows — is
        // checked here, before any HIP call: this also keeps an absurd max_batch (a corrupted settings value) from the allocator
        const auto too_large = [&](size_t per_board) {
            const size_t limit = (((size_t)1 << 31) - 1) / std::max<size_t>(per_board, 1);
            return (size_t)max_batch > limit && fail("kz_engine_create: max_batch " + std::to_string(max_batch) + " too large for this "
                                                     "network: at most " + std::to_string(limit) + " boards (every engine tensor must stay below 2 GiB)");
        };
        const Model &mm = *model->m;
        if (too_large((size_t)4 * std::max<size_t>((size_t)mm.h * mm.w * round_up(std::max(mm.channels, mm.c_in), 64),
                                                   (size_t)std::max(mm.policy_len, 1))))
            return 1;
        if (!known_dtype(dtype)) return fail("kz_engine_create: unknown dtype");
        // KZ_DTYPE_F32_SPLIT16 and bf16 are the f32 engine with one kernel exchanged: everything below sees KZ_DTYPE_F32
        const int dtype_in = dtype;
        if (dtype == KZ_DTYPE_F32_SPLIT16 || dtype == KZ_DTYPE_BF16) dtype = KZ_DTYPE_F32;
        if (int8_dtype(dtype)) dtype = KZ_DTYPE_F16;  // ... and int8 (4, 5) is the f16 engine with the tower's launch exchanged
        int ndev = 0;
        HIP_TRY(hipGetDeviceCount(&ndev));
        if (device < 0 || device >= ndev)
            return fail("kz_engine_create: device " + std::to_string(device) + " out of range (" + std::to_string(ndev) +
                        " visible)");
        HIP_TRY(hipSetDevice(device));

        std::unique_ptr<kz_engine, void (*)(kz_engine *)> e(new kz_engine(), kz_engine_destroy);
        e->model = profile != Profile::none && profile != Profile::taps ? model->m : effective_model(model, dtype_in, max_batch);
        e->source_model = model->m;
        e->out_channels = model->m->channels;
        const Model &m = *e->model;
        e->device = device;
        e->dtype = dtype;
        e->created_dtype = dtype_in;
        e->max_batch = max_batch;
        e->esz = dtype == KZ_DTYPE_F32 ? 4 : 2;
        e->cin_p = round_up(m.c_in, 32);
        e->cp = round_up(m.channels, 32);
        // which kernels run this network: plan_path (kz_plan.hpp) — the table of DESIGN.md §5 is printed from it
        std::string why;
        if (profile_per_layer(profile)) {
            e->plan = PathPlan();  // (Tower::conv_igemm)
            e->plan.keep = true;
            e->plan.launches = 2 + 2 * m.depth;
        } else if (profile == Profile::taps) {  // (the caller has asked plan_path already: a one-launch ResTower, or an int8 plan)
            if (!plan_path(m, max_batch, dtype_in, e->plan, why)) return fail("kz_engine_create: " + why);
            e->plan.heads = false;
            e->plan.launches = 1;
        } else if (profile != Profile::none) {
            e->plan = PathPlan();
            e->plan.tower = Tower::resident_f32;
            e->plan.launches = 1;
        } else {
            if (!plan_path(m, max_batch, dtype_in, e->plan, why)) return fail("kz_engine_create: " + why);
            experiment_switches(m, dtype, e->cin_p, e->plan);
        }
        const PathPlan &plan = e->plan;
        {
            std::lock_guard<std::mutex> lock(g_cache_mutex);
            const WeightsKey key{e->model.get(), device, dtype, weights_spec(m, plan)};
            auto it = g_cache.find(key);
            if (it != g_cache.end()) e->wts = it->second.lock();
            if (!e->wts) {
                auto w = std::make_shared<DeviceWeights>();
                w->device = device;
                w->dtype = dtype;
                if (w->build(m, key.spec)) return 1;
                g_cache[key] = w;
                e->wts = w;
            }
        }
        // head temporaries, for run_heads' separate launches: the one tensor pair the check above does not bound
        const size_t hw = (size_t)m.h * m.w, rows = (size_t)max_batch * hw;
        size_t h0 = 0, h1 = 0;
        const DeviceWeights &w = *e->wts;
        if (!plan.heads && !plan.att_heads) switch (m.policy_kind) {
            case kz::POLICY_ATAXX_CONV:
            case kz::POLICY_ARIMAA:
            case kz::POLICY_CONV: h0 = rows * w.pol.conv0.cout_p; break;
            case kz::POLICY_ATTENTION:
                h0 = rows * w.pol.bulk.cout_p;
                h1 = (size_t)max_batch * 8 * w.pol.under.cout_p;
                break;
            case kz::POLICY_NONE: break;
            case kz::POLICY_DENSE:
                if (m.dense_hidden_channels) h0 = rows * w.pol.conv0.cout_p;
                if (m.dense_hidden_size) h1 = (size_t)max_batch * w.pol.fc0.cout_p;
                break;
        }
        if (too_large(std::max(h0, h1) * e->esz / max_batch)) return 1;

        HIP_TRY(hipStreamCreateWithFlags(&e->slot_stream[0], hipStreamNonBlocking));
        if (plan.heads) {  // one launch per batch that touches nothing but its slot's buffers
            HIP_TRY(hipStreamCreateWithFlags(&e->slot_stream[1], hipStreamNonBlocking));
            for (int i = 2; i < KZ_ENGINE_SLOTS; i++) e->slot_stream[i] = e->slot_stream[i & 1];
            e->zero_copy = true;
    #ifdef KZ_EXPERIMENTS
            e->zero_copy = !plan.no_zero_copy;
    #endif
        }
        if (e->wts->stem_cin_p) e->cin_p = e->wts->stem_cin_p;
        if (e->dmalloc(&e->x_in, rows * e->cin_p * e->esz)) return 1;
    #ifdef KZ_EXPERIMENTS
        if (plan.nb4 && e->dmalloc(&e->xres, kz::tower4_scratch_bytes(max_batch))) return 1;
    #endif
        for (int i = 0; i < (per_layer(plan) ? 3 : 1); i++)
            if (e->dmalloc(&e->act[i], rows * e->cp * e->esz)) return 1;
        if (plan.tower == Tower::board_conv_i8) {  // (within the 2 GiB bound checked above: C8 <= 4 * round_up(channels, 64))
            for (int i = 0; i < 2; i++)
                if (e->dmalloc(&e->act8[i], rows * e->wts->c8)) return 1;
        }
        if (e->dmalloc(&e->head0, h0 * e->esz) || e->dmalloc(&e->head1, h1 * e->esz)) return 1;

        const int nb_planes = m.n_bool < 0 ? 0 : m.n_bool, ns_planes = m.n_scalar < 0 ? 0 : m.n_scalar;
        const size_t bits_bytes = (size_t)(nb_planes * hw + 7) / 8;
        // every flag word a launch is handed has the range check's per-board words in front of it (kz_engine_state.hpp: Slot)
        const size_t front = (size_t)e->front_words();
        for (auto &s : e->slots) {
            float *d_base = nullptr, *h_base = nullptr;
            if (e->dmalloc((void **)&s.d_bits, max_batch * bits_bytes) ||
                e->dmalloc((void **)&s.d_sin, (size_t)max_batch * ns_planes * 4) ||
                e->dmalloc((void **)&d_base, (front + (size_t)max_batch * 5 + kz_engine::SOUT_HDR) * 4) ||
                e->dmalloc((void **)&s.d_pol, (size_t)max_batch * m.policy_len * 4))
                return 1;
            if (e->hmalloc((void **)&s.h_bits, max_batch * bits_bytes) ||
                e->hmalloc((void **)&s.h_sin, (size_t)max_batch * ns_planes * 4) ||
                e->hmalloc((void **)&h_base, (front + (size_t)max_batch * 5 + kz_engine::SOUT_HDR) * 4) ||
                e->hmalloc((void **)&s.h_pol, (size_t)max_batch * m.policy_len * 4))
                return 1;
            HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
            HIP_TRY(hipMemset(d_base, 0, (front + kz_engine::SOUT_HDR) * 4));
            memset(h_base, 0, (front + kz_engine::SOUT_HDR) * 4);
            s.d_sout = d_base + front;
            s.h_sout = h_base + front;
            s.status.assign((size_t)max_batch, 0);
        }
        int *devflag_base = nullptr;
        if (e->dmalloc((void **)&devflag_base, (front + 4) * 4)) return 1;
        HIP_TRY(hipMemset(devflag_base, 0, (front + 4) * 4));
        e->d_devflag = devflag_base + front;
        if (profile_hist(profile)) {
            const size_t bytes = (size_t)(2 * m.depth + 1) * kz::RANGE_BINS * sizeof(unsigned long long);
            if (e->dmalloc(&e->range_out, bytes)) return 1;
            HIP_TRY(hipMemset(e->range_out, 0, bytes));
            e->range_hist = true;
        } else if (profile_taps(profile)) {
            // every site's tensor for tap_boards boards, all of them together below 2 GiB
            const size_t per_board = (size_t)(2 * m.depth + 1) * hw * m.channels * 4;
            e->tap_boards = (int)std::min<size_t>((size_t)std::min(max_batch, std::max(tap_boards, 1)), std::max<size_t>(((((size_t)1 << 31) - 1) / per_board), 1));
            // (board_conv_i8: a site's halves hold the engine's own rows, C8 bytes and cp f16 values — kz_engine_state.hpp, tap_copy)
            if (plan.tower == Tower::board_conv_i8 && (e->wts->c8 > 2 * m.channels || e->cp > m.channels))
                return fail("kz_engine_create: internal error: the per-layer int8 rows do not fit the tap tensors of this shape");
            if (e->dmalloc((void **)&e->tap_out, per_board * e->tap_boards)) return 1;
        } else if ((profile == Profile::per_layer || profile == Profile::resident) &&
                   e->dmalloc(&e->range_out, (size_t)(2 * m.depth + 1) * max_batch * 4)) {
            return 1;
        }
        *out = e.release();
        return 0;
    }
}

KZ_API int kz_engine_create(const kz_model *model, int device, int max_batch, int dtype, kz_engine **out) {
    return guarded("kz_engine_create", [&]() -> int { return create_engine(model, device, max_batch, dtype, Profile::none, out); });
}

KZ_API int kz_model_supports_dtype(const kz_model *model, int dtype) {
    return guarded("kz_model_supports_dtype", [&]() -> int {
        if (!model) return -1;
        if (!known_dtype(dtype)) return -1;
        // (larger boards in split arithmetic run per layer: the engine additionally needs max_batch * h * w * channels * 4 bytes
        // < 2 GiB, asked here for one board)
        PathPlan plan;
        std::string why;
        return plan_path(*effective_model(model, dtype, 1), 1, dtype, plan, why) ? 1 : 0;
    }, -1);
}

KZ_API int kz_model_plan(const kz_model *model, int max_batch, int dtype, kz_path_plan *out) {
    return guarded("kz_model_plan", [&]() -> int {
        if (!model || !out) return fail("kz_model_plan: null argument");
        if (max_batch <= 0) return fail("kz_model_plan: max_batch must be positive");
        if (!known_dtype(dtype)) return fail("kz_model_plan: unknown dtype");
        PathPlan plan;
        std::string why;
        if (!plan_path(*effective_model(model, dtype, max_batch), max_batch, dtype, plan, why)) return fail("kz_model_plan: " + why);
        memset(out, 0, sizeof *out);
        snprintf(out->tower_path, sizeof out->tower_path, "%s", path_name(plan, dtype));
        out->launches_per_batch = plan.launches;
        return 0;
    });
}

KZ_API int kz_model_launch_geometry(const kz_model *model, int max_batch, int dtype, int batch, int *workgroups, int *boards_per_workgroup) {
    return guarded("kz_model_launch_geometry", [&]() -> int {
        if (!model || !workgroups || !boards_per_workgroup) return fail("kz_model_launch_geometry: null argument");
        if (max_batch <= 0) return fail("kz_model_launch_geometry: max_batch must be positive");
        if (!known_dtype(dtype)) return fail("kz_model_launch_geometry: unknown dtype");
        if (batch < 0 || batch > max_batch) return fail("kz_model_launch_geometry: batch out of range");
        const std::shared_ptr<Model> m = effective_model(model, dtype, max_batch);
        PathPlan plan;
        std::string why;
        if (!plan_path(*m, max_batch, dtype, plan, why)) return fail("kz_model_launch_geometry: " + why);
        // (what kz_engine_create makes of the dtype: split16 and bf16 are the f32 engine, int8 the f16 engine)
        const int engine_dtype = dtype == KZ_DTYPE_F32_SPLIT16 || dtype == KZ_DTYPE_BF16 ? KZ_DTYPE_F32 : int8_dtype(dtype) ? KZ_DTYPE_F16 : dtype;
        experiment_switches(*m, engine_dtype, round_up(m->c_in, 32), plan);
        launch_geometry_of(*m, plan, engine_dtype, batch, workgroups, boards_per_workgroup);
        return 0;
    });
}

// ------------------------------------------------------------------------------------------------
// Stream shift and range profile: the same function with a residual stream 2^-k times as large (kz::stream_shift), and how
// large the stored tower tensors of a network are on the caller's positions, measured in exact f32
// ------------------------------------------------------------------------------------------------
KZ_API int kz_model_quantize_int8(const kz_model *model, const float *site_max, int n_sites, kz_model **out) {
    return guarded("kz_model_quantize_int8", [&]() -> int {
        if (!model || !site_max || !out) return fail("kz_model_quantize_int8: null argument");
        std::string err;
        Model *m = kz::quantize_int8(*model->m, site_max, n_sites, err);
        if (!m) return fail("kz_model_quantize_int8: " + err);
        *out = new kz_model(std::shared_ptr<Model>(m));
        return 0;
    });
}

KZ_API int kz_model_int8_site_exponents(const kz_model *model, int *exp_out) {
    return guarded("kz_model_int8_site_exponents", [&]() -> int {
        if (!model || !exp_out) return fail("kz_model_int8_site_exponents: null argument");
        const Model &m = *model->m;
        if (m.i8_exp.empty()) return fail("kz_model_int8_site_exponents: this model is not calibrated (kz_model_quantize_int8 makes one that is)");
        std::copy(m.i8_exp.begin(), m.i8_exp.end(), exp_out);
        return 0;
    });
}

KZ_API int kz_model_stream_shift(const kz_model *model, int k, kz_model **out) {
    return guarded("kz_model_stream_shift", [&]() -> int {
        if (!model || !out) return fail("kz_model_stream_shift: null argument");
        std::string err;
        Model *m = kz::stream_shift(*model->m, k, err);
        if (!m) return fail("kz_model_stream_shift: " + err);
        *out = new kz_model(std::shared_ptr<Model>(m));
        return 0;
    });
}

// the sites exist for a ResTower with at least one block: 2 * depth + 1 of them, in run_tower's stash order
static int range_site_count(const char *fn, const kz_model *model, int &n) {
    if (!model) return fail(std::string(fn) + ": null argument");
    const Model &m = *model->m;
    if (m.tower_kind != kz::TOWER_RES) return fail(std::string(fn) + ": the range sites are a ResTower's (this network has none)");
    if (m.depth < 1) return fail(std::string(fn) + ": a tower without blocks has no residual stream to profile");
    n = 2 * m.depth + 1;
    return 0;
}

KZ_API int kz_model_range_sites(const kz_model *model, int *n_sites) {
    return guarded("kz_model_range_sites", [&]() -> int {
        int n = 0;
        if (range_site_count("kz_model_range_sites", model, n)) return 1;
        if (!n_sites) return fail("kz_model_range_sites: null argument");
        *n_sites = n;
        return 0;
    });
}

KZ_API int kz_model_range_site_name(const kz_model *model, int site, char *buf, size_t len) {
    return guarded("kz_model_range_site_name", [&]() -> int {
        int n = 0;
        if (range_site_count("kz_model_range_site_name", model, n)) return 1;
        if (site < 0 || site >= n) return fail("kz_model_range_site_name: site " + std::to_string(site) + " out of range (" + std::to_string(n) + " sites)");
        // site 0: the stem; 2i - 1: block i's mid activation; 2i: block i's output, the last one behind the final BN
        const std::string name = site == 0       ? "tower.0"
                                 : site % 2      ? "tower." + std::to_string((site + 1) / 2) + ".mid"
                                 : site == n - 1 ? "tower." + std::to_string(site / 2 + 1)
                                                 : "tower." + std::to_string(site / 2);
        if (!buf || len < name.size() + 1) return fail("kz_model_range_site_name: buffer of at least " + std::to_string(name.size() + 1) + " bytes needed");
        memcpy(buf, name.c_str(), name.size() + 1);
        return 0;
    });
}

// where kz_model_range_profile_fast runs: the one-launch exact-f32 tower wherever the kernel takes the shape
static bool range_profile_resident(const Model &m) { return kz::tower32_supported(KZ_DTYPE_F32, m.h, m.w, m.channels, m.depth); }

// the profile and histogram entries: an internal engine of `mode` with max_batch = min(batch, chunk_max), the boards in chunks
// of that.  A histogram mode fills hist_out [n_sites][KZ_RANGE_BINS] — the engine's counters add up over the chunks and are
// read once — and the two maxima pointers are null.
static_assert(KZ_RANGE_BINS == kz::RANGE_BINS, "the kernels' bins are the header's");
static int range_profile(const std::string &fn, Profile mode, int chunk_max, const kz_model *model, int device, const uint8_t *bits,
                         size_t bits_stride, const float *scalars_in, int batch, float *site_max_out, float *board_max_out,
                         uint64_t *hist_out = nullptr) {
    const bool hist = profile_hist(mode);
    int n = 0;
    if (range_site_count(fn.c_str(), model, n)) return 1;
    const Model &m = *model->m;
    if (m.n_scalar < 0) return fail(no_plane_split(fn));
    if (batch < 1) return fail(fn + ": batch must be positive");
    if (!bits || (m.n_scalar && !scalars_in) || !(hist ? (const void *)hist_out : (const void *)site_max_out)) return fail(fn + ": null argument");
    if (bits_stride < bits_bytes(m)) return fail(fn + ": bits_stride too small");
    const int chunk = std::min(batch, chunk_max);
    kz_engine *raw = nullptr;
    // (a histogram entry's every failure is in its own name; the maxima entries keep the engine's message as it is)
    if (create_engine(model, device, chunk, KZ_DTYPE_F32, mode, &raw)) return hist ? fail(fn + ": " + std::string(g_err)) : 1;
    std::unique_ptr<kz_engine, void (*)(kz_engine *)> e(raw, kz_engine_destroy);
    kz_engine::Slot &s = e->slots[0];
    std::vector<float> host(hist ? 0 : (size_t)n * chunk);
    for (int i = 0; i < n && !hist; i++) site_max_out[i] = 0.0f;
    // (the kernel's values are never NaN: a non-finite board reports +inf)
    for (int lo = 0; lo < batch; lo += chunk) {
        const int nb = std::min(chunk, batch - lo);
        e->stage_boards(s, bits + (size_t)lo * bits_stride, bits_stride, m.n_scalar ? scalars_in + (size_t)lo * m.n_scalar : nullptr, nb);
        const Pass p = e->pass_staged(0);
        if (e->copy_boards_in(p, s, nb)) return 1;
        // the tower only: the heads read nothing the profile reports
        const kz::PackedBoards in = e->packed_boards(s.d_bits, e->bits_bytes(), s.d_sin);
        if (!profile_per_layer(mode)) {  // one launch: encode, tower and the maxima
            if (e->run_tower(p, nb, s.d_sout + kz_engine::SOUT_HDR, s.d_pol, &in)) return 1;
        } else {
            if (e->launch(p, "kz_encode_packed", [&] { kz::launch_encode_packed(e->dtype, in, nb, m.h * m.w, e->x_in, e->cin_p, p.stream); }))
                return 1;
            if (e->run_tower(p, nb, s.d_sout + kz_engine::SOUT_HDR, s.d_pol)) return 1;
        }
        if (e->range_site != n) return fail(fn + ": internal error: " + std::to_string(e->range_site) + " sites measured, " + std::to_string(n) + " expected");
        if (!hist) HIP_TRY(hipMemcpyAsync(host.data(), e->range_out, host.size() * 4, hipMemcpyDeviceToHost, p.stream));
        HIP_TRY(hipStreamSynchronize(p.stream));  // (the staging is free for the next chunk)
        if (hist) continue;
        for (int b = 0; b < nb; b++) {
            // behind a non-finite tensor the values are not the network's (ReLU turns a NaN into 0): the board reports +inf
            // from its first non-finite site on
            bool nonfinite = false;
            for (int i = 0; i < n; i++) {
                nonfinite = nonfinite || host[(size_t)i * chunk + b] == INFINITY;
                const float v = nonfinite ? INFINITY : host[(size_t)i * chunk + b];
                site_max_out[i] = std::max(site_max_out[i], v);
                if (board_max_out && i < n - 1) board_max_out[lo + b] = i == 0 ? v : std::max(board_max_out[lo + b], v);
            }
        }
    }
    if (hist) {
        static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the counters");
        const size_t bytes = (size_t)n * kz::RANGE_BINS * sizeof(uint64_t);
        HIP_TRY(hipMemcpy(hist_out, e->range_out, bytes, hipMemcpyDeviceToHost));
    }
    return 0;
}

KZ_API int kz_model_range_profile(const kz_model *model, int device, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                                  int batch, float *site_max_out, float *board_max_out) {
    return guarded("kz_model_range_profile", [&]() -> int {
        return range_profile("kz_model_range_profile", Profile::per_layer, 64, model, device, bits, bits_stride, scalars_in, batch,
                             site_max_out, board_max_out);
    });
}

KZ_API int kz_model_range_profile_fast(const kz_model *model, int device, const uint8_t *bits, size_t bits_stride,
                                       const float *scalars_in, int batch, float *site_max_out, float *board_max_out) {
    return guarded("kz_model_range_profile_fast", [&]() -> int {
        const std::string fn = "kz_model_range_profile_fast";
        int n = 0;
        if (range_site_count(fn.c_str(), model, n)) return 1;
        // elsewhere (Go 19x19, other widths): exactly the per-layer profile
        const bool resident = range_profile_resident(*model->m);
        return range_profile(fn, resident ? Profile::resident : Profile::per_layer, resident ? 256 : 64, model, device, bits, bits_stride,
                             scalars_in, batch, site_max_out, board_max_out);
    });
}

KZ_API int kz_model_range_histogram(const kz_model *model, int device, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                                    int batch, void *hist_out) {
    return guarded("kz_model_range_histogram", [&]() -> int {
        return range_profile("kz_model_range_histogram", Profile::per_layer_hist, 64, model, device, bits, bits_stride, scalars_in, batch,
                             nullptr, nullptr, (uint64_t *)hist_out);
    });
}

KZ_API int kz_model_range_histogram_fast(const kz_model *model, int device, const uint8_t *bits, size_t bits_stride,
                                         const float *scalars_in, int batch, void *hist_out) {
    return guarded("kz_model_range_histogram_fast", [&]() -> int {
        const std::string fn = "kz_model_range_histogram_fast";
        int n = 0;
        if (range_site_count(fn.c_str(), model, n)) return 1;
        const bool resident = range_profile_resident(*model->m);
        return range_profile(fn, resident ? Profile::resident_hist : Profile::per_layer_hist, resident ? 256 : 64, model, device, bits,
                             bits_stride, scalars_in, batch, nullptr, nullptr, (uint64_t *)hist_out);
    });
}

KZ_API int kz_model_range_profile_fast_path(const kz_model *model, char *buf, size_t len) {
    return guarded("kz_model_range_profile_fast_path", [&]() -> int {
        int n = 0;
        if (range_site_count("kz_model_range_profile_fast_path", model, n)) return 1;
        const std::string name = range_profile_resident(*model->m) ? "tower_resident_f32" : "conv_igemm_f32";
        if (!buf || len < name.size() + 1)
            return fail("kz_model_range_profile_fast_path: buffer of at least " + std::to_string(name.size() + 1) + " bytes needed");
        memcpy(buf, name.c_str(), name.size() + 1);
        return 0;
    });
}

// ------------------------------------------------------------------------------------------------
// Tower taps and error profile (include/kz_hip.h): every stored tensor of the one-launch tower an engine of (max_batch, dtype)
// runs, as the kernel rounds it, and its deviation from exact f32 per site
// ------------------------------------------------------------------------------------------------

// What a tap call runs: kz_model_plan's tower for (max_batch, dtype), never with the heads inside.  Host logic only (plan_path),
// so every refusal below needs no GPU.  n: the range sites.
static int tap_plan(const std::string &fn, const kz_model *model, int max_batch, int dtype, PathPlan &plan, int &n) {
    if (!model) return fail(fn + ": null argument");
    const Model &m = *model->m;
    if (m.tower_kind == kz::TOWER_ATTENTION)
        return fail(fn + ": an AttentionTower network has no range sites to tap: the taps are the one-launch ResTower's stored tensors");
    if (m.tower_kind == kz::TOWER_DENSE_NET) return fail(fn + ": a DenseNetwork has no tower, and its one launch has no tap instance");
    if (m.depth < 1) return fail(fn + ": a tower without blocks has no residual stream to tap");
    n = 2 * m.depth + 1;
    if (max_batch <= 0) return fail(fn + ": max_batch must be positive");
    if (!known_dtype(dtype)) return fail(fn + ": unknown dtype " + std::to_string(dtype));
    if (int8_dtype(dtype)) return fail(fn + ": the int8 tower (dtype " + std::to_string(dtype) + ") has no tap instance: its stored tensors are int8 images at a scale per site, which the taps' element formats do not hold");
    std::string why;
    if (!plan_path(*effective_model(model, dtype, max_batch), max_batch, dtype, plan, why))
        return fail(fn + ": this model does not run in dtype " + std::to_string(dtype) + ": " + why);
    if (per_layer(plan))
        return fail(fn + ": at max_batch " + std::to_string(max_batch) + " this network runs one launch per layer (" + path_name(plan, dtype) +
                    "), which keeps its activations in device memory already: read those with KZ_KEEP_ACTIVATIONS=1 and "
                    "kz_engine_read_activation; the taps are the one-launch towers'");
    plan.heads = false;
    return 0;
}

// the argument checks the two evaluating entries share, after tap_plan
static int tap_arguments(const std::string &fn, const Model &m, int max_batch, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                         int batch) {
    if (m.n_scalar < 0) return fail(no_plane_split(fn));
    if (m.n_scalar && !scalars_in) return fail(fn + ": null argument");
    if (batch < 1 || batch > max_batch)
        return fail(fn + ": batch " + std::to_string(batch) + " out of range: 1 .. max_batch (" + std::to_string(max_batch) + "), the batch size whose geometry is tapped");
    if (bits_stride < bits_bytes(m)) return fail(fn + ": bits_stride too small (" + std::to_string(bits_stride) + " < " + std::to_string(bits_bytes(m)) + " bytes per board)");
    return 0;
}

using EnginePtr = std::unique_ptr<kz_engine, void (*)(kz_engine *)>;
static int tap_engine(const std::string &fn, const kz_model *model, int device, int max_batch, int dtype, Profile mode, int tap_boards, EnginePtr &e) {
    kz_engine *raw = nullptr;
    if (create_engine(model, device, max_batch, dtype, mode, &raw, tap_boards)) return fail(fn + ": " + std::string(g_err));
    e.reset(raw);
    return 0;
}

// one pass of a tap engine over nb <= tap_boards boards: the tap buffer to NaN patterns, then the launch; returns with the
// stream idle
static int tap_pass(kz_engine *e, const uint8_t *bits, size_t bits_stride, const float *scalars_in, int nb) {
    kz_engine::Slot &s = e->slots[0];
    const Model &m = *e->model;
    e->stage_boards(s, bits, bits_stride, scalars_in, nb);
    const Pass p = e->pass_staged(0);
    if (e->copy_boards_in(p, s, nb)) return 1;
    if (e->tap_fill(p)) return 1;  // (an int8 tap engine: 0x80 in the image parts)
    const kz::PackedBoards in = e->packed_boards(s.d_bits, e->bits_bytes(), s.d_sin);
    e->range_site = 0;
    if (per_layer(e->plan)) {  // (board_conv_i8: the encode is a launch of its own)
        if (e->launch(p, "kz_encode_packed", [&] { kz::launch_encode_packed(e->dtype, in, nb, m.h * m.w, e->x_in, e->cin_p, p.stream); })) return 1;
        if (e->run_tower(p, nb, s.d_sout + kz_engine::SOUT_HDR, s.d_pol)) return 1;
    } else if (e->run_tower(p, nb, s.d_sout + kz_engine::SOUT_HDR, s.d_pol, &in)) {
        return 1;
    }
    if (e->range_site != 2 * m.depth + 1) return fail("internal error: the planned tower has no tap instance");
    HIP_TRY(hipStreamSynchronize(p.stream));
    return 0;
}

KZ_API int kz_model_tower_taps_path(const kz_model *model, int max_batch, int dtype, char *buf, size_t len) {
    return guarded("kz_model_tower_taps_path", [&]() -> int {
        const std::string fn = "kz_model_tower_taps_path";
        PathPlan plan;
        int n = 0;
        if (tap_plan(fn, model, max_batch, dtype, plan, n)) return 1;
        const std::string name = path_name(plan, dtype);
        if (!buf || len < name.size() + 1) return fail(fn + ": buffer of at least " + std::to_string(name.size() + 1) + " bytes needed");
        memcpy(buf, name.c_str(), name.size() + 1);
        return 0;
    });
}

KZ_API int kz_model_tower_taps(const kz_model *model, int device, int max_batch, int dtype, const uint8_t *bits, size_t bits_stride,
                               const float *scalars_in, int batch, int site_first, int n_sites, float *out) {
    return guarded("kz_model_tower_taps", [&]() -> int {
        const std::string fn = "kz_model_tower_taps";
        if (!model || !bits || !out) return fail(fn + ": null argument");
        PathPlan plan;
        int n = 0;
        if (tap_plan(fn, model, max_batch, dtype, plan, n)) return 1;
        if (site_first < 0 || n_sites < 1 || site_first > n - n_sites)
            return fail(fn + ": sites [" + std::to_string(site_first) + ", " + std::to_string((long long)site_first + n_sites) + ") out of range (" +
                        std::to_string(n) + " sites)");
        const Model &src = *model->m;
        if (tap_arguments(fn, src, max_batch, bits, bits_stride, scalars_in, batch)) return 1;
        EnginePtr e(nullptr, kz_engine_destroy);
        if (tap_engine(fn, model, device, max_batch, dtype, Profile::taps, batch, e)) return 1;
        // The host loop converts: a site's rows come back as the kernel stored them (NHWC, the site's element) and are widened
        // and transposed here — no second device tensor, and this is no hot path.  (e->model may be the widened network: its
        // zero channels behind the model's own are not returned.)
        const size_t hw = (size_t)src.h * src.w, ld = (size_t)e->model->channels, channels = (size_t)e->out_channels;
        std::vector<unsigned char> host((size_t)e->tap_boards * hw * ld * 4);
        for (int lo = 0; lo < batch; lo += e->tap_boards) {
            const int nb = std::min(e->tap_boards, batch - lo);
            if (tap_pass(e.get(), bits + (size_t)lo * bits_stride, bits_stride, src.n_scalar ? scalars_in + (size_t)lo * src.n_scalar : nullptr, nb))
                return fail(fn + ": " + std::string(g_err));
            const size_t rows = (size_t)nb * hw;
            for (int si = 0; si < n_sites; si++) {
                const int site = site_first + si;
                const kz::TapFormat f = e->tap_format(site);
                const size_t esz = f == kz::TapFormat::f32 ? 4 : 2;
                HIP_TRY(hipMemcpy(host.data(), e->tap_site(site), rows * ld * esz, hipMemcpyDeviceToHost));
                if (f == kz::TapFormat::split16)
                    HIP_TRY(hipMemcpy(host.data() + rows * ld * 2, e->tap_site(site) + e->tap_site_bytes() / 2, rows * ld * 2, hipMemcpyDeviceToHost));
                const float *h32 = reinterpret_cast<const float *>(host.data());
                const _Float16 *h16 = reinterpret_cast<const _Float16 *>(host.data()), *l16 = h16 + rows * ld;
                const uint16_t *b16 = reinterpret_cast<const uint16_t *>(host.data());
                for (size_t r = 0; r < rows; r++) {
                    float *dst = out + (((size_t)si * batch + lo) * channels) * hw + (r / hw) * channels * hw + r % hw;
                    for (size_t c = 0; c < channels; c++) {
                        const size_t i = r * ld + c;
                        float v;
                        if (f == kz::TapFormat::f32) v = h32[i];
                        else if (f == kz::TapFormat::f16) v = (float)h16[i];
                        else if (f == kz::TapFormat::split16) v = (float)h16[i] + (float)l16[i];
                        else {
                            const uint32_t u = (uint32_t)b16[i] << 16;
                            memcpy(&v, &u, 4);
                        }
                        dst[c * hw] = v;
                    }
                }
            }
        }
        return 0;
    });
}

static_assert(sizeof(kz_site_error) == 48 && sizeof(kz::TapDeviation) == sizeof(kz_site_error), "a device record is a kz_site_error: the two maxima as the bit patterns of non-negative doubles");
KZ_API int kz_model_error_profile(const kz_model *model, int device, int max_batch, int dtype, const uint8_t *bits, size_t bits_stride,
                                  const float *scalars_in, int batch, void *out) {
    return guarded("kz_model_error_profile", [&]() -> int {
        const std::string fn = "kz_model_error_profile";
        if (!model || !bits || !out) return fail(fn + ": null argument");
        PathPlan plan;
        int n = 0;
        if (tap_plan(fn, model, max_batch, dtype, plan, n)) return 1;
        if (dtype == KZ_DTYPE_F32) return fail(fn + ": KZ_DTYPE_F32 is the reference: a profile of exact f32 against itself compares nothing");
        const Model &src = *model->m;
        if (tap_arguments(fn, src, max_batch, bits, bits_stride, scalars_in, batch)) return 1;
        // the reference: the one-launch f32 tower's own taps where that kernel takes the shape, else the per-layer exact-f32
        // engine (kz_model_range_profile's), whose stash sites are compared as they are produced
        const bool resident = range_profile_resident(src);
        EnginePtr e(nullptr, kz_engine_destroy), ref(nullptr, kz_engine_destroy);
        if (tap_engine(fn, model, device, max_batch, dtype, Profile::taps, resident ? batch : std::min(batch, 64), e)) return 1;
        const int chunk = std::min(batch, e->tap_boards);
        if (tap_engine(fn, model, device, chunk, KZ_DTYPE_F32, resident ? Profile::taps_reference : Profile::per_layer_deviation, chunk, ref)) return 1;
        kz::TapDeviation *dev = nullptr;
        if (e->dmalloc((void **)&dev, (size_t)n * sizeof(kz::TapDeviation))) return fail(fn + ": " + std::string(g_err));
        HIP_TRY(hipMemset(dev, 0, (size_t)n * sizeof(kz::TapDeviation)));
        HIP_TRY(hipDeviceSynchronize());  // (the engines' streams do not wait for the null stream)
        if (!resident) {
            ref->tap_peer = e.get();
            ref->deviation = dev;
        }
        for (int lo = 0; lo < batch; lo += chunk) {
            const int nb = std::min(chunk, batch - lo);
            const uint8_t *b = bits + (size_t)lo * bits_stride;
            const float *sc = src.n_scalar ? scalars_in + (size_t)lo * src.n_scalar : nullptr;
            if (tap_pass(e.get(), b, bits_stride, sc, nb)) return fail(fn + ": " + std::string(g_err));
            if (resident) {
                if (tap_pass(ref.get(), b, bits_stride, sc, nb)) return fail(fn + ": " + std::string(g_err));
                const Pass p = ref->pass_staged(0);
                for (int site = 0; site < n; site++)
                    if (e->tap_deviation(p, site, reinterpret_cast<const float *>(ref->tap_site(site)), ref->model->channels, nb, dev + site))
                        return fail(fn + ": " + std::string(g_err));
                HIP_TRY(hipStreamSynchronize(p.stream));
            } else {
                kz_engine::Slot &s = ref->slots[0];
                ref->stage_boards(s, b, bits_stride, sc, nb);
                const Pass p = ref->pass_staged(0);
                if (ref->copy_boards_in(p, s, nb)) return fail(fn + ": " + std::string(g_err));
                const kz::PackedBoards in = ref->packed_boards(s.d_bits, ref->bits_bytes(), s.d_sin);
                if (ref->launch(p, "kz_encode_packed", [&] { kz::launch_encode_packed(ref->dtype, in, nb, src.h * src.w, ref->x_in, ref->cin_p, p.stream); }) ||
                    ref->run_tower(p, nb, s.d_sout + kz_engine::SOUT_HDR, s.d_pol))
                    return fail(fn + ": " + std::string(g_err));
                if (ref->range_site != n) return fail(fn + ": internal error: " + std::to_string(ref->range_site) + " sites compared, " + std::to_string(n) + " expected");
                HIP_TRY(hipStreamSynchronize(p.stream));
            }
        }
        HIP_TRY(hipMemcpy(out, dev, (size_t)n * sizeof(kz_site_error), hipMemcpyDeviceToHost));
        return 0;
    });
}

// ------------------------------------------------------------------------------------------------
// Int8 taps and error profile (include/kz_hip.h): every stored int8 image of the int8 tower an engine of (max_batch, dtype)
// runs, the f16 stream value stored beside it, and per site the error of both against exact f32 with the clamp counts
// ------------------------------------------------------------------------------------------------

// What an int8 tap call runs: host logic only.  tap_dtype: the dtype of the tap engine — dtype 5 taps what dtype 4 taps (the
// tower's bits are dtype 4's, and a tap engine carries no heads: its wide levels are the tower's own), dtype 8 that tower
// wherever dtype 5 has a plan and the per-layer kernel elsewhere.
static int int8_tap_plan(const std::string &fn, const kz_model *model, int max_batch, int dtype, PathPlan &plan, int &n, int &tap_dtype) {
    if (!model) return fail(fn + ": null argument");
    if (!int8_dtype(dtype)) return fail(fn + ": dtype " + std::to_string(dtype) + " is not an int8 dtype (4, 5 or 8): kz_model_tower_taps and kz_model_error_profile take the others");
    const Model &m = *model->m;
    if (m.tower_kind == kz::TOWER_ATTENTION) return fail(fn + ": an AttentionTower network has no range sites to tap, and no int8 arithmetic");
    if (m.tower_kind == kz::TOWER_DENSE_NET) return fail(fn + ": a DenseNetwork has no tower, and no int8 arithmetic");
    if (m.depth < 1) return fail(fn + ": a tower without blocks has no quantised image to tap");
    n = 2 * m.depth + 1;
    if (max_batch <= 0) return fail(fn + ": max_batch must be positive");
    if (m.i8_exp.empty())
        return fail(fn + ": this model is not calibrated (kz_model_quantize_int8 makes one that is): an int8 image of dtype " + std::to_string(dtype) + " has a scale per site");
    std::string why;
    if (!plan_path(*effective_model(model, dtype, max_batch), max_batch, dtype, plan, why))
        return fail(fn + ": this model does not run in dtype " + std::to_string(dtype) + ": " + why);
    tap_dtype = dtype;
    if (plan.tower == Tower::resident_i8) {
        tap_dtype = KZ_DTYPE_INT8;
        if (!plan_path(*effective_model(model, tap_dtype, max_batch), max_batch, tap_dtype, plan, why)) return fail(fn + ": internal error: " + why);
    }
    plan.heads = false;
    return 0;
}

KZ_API int kz_model_int8_taps_path(const kz_model *model, int max_batch, int dtype, char *buf, size_t len) {
    return guarded("kz_model_int8_taps_path", [&]() -> int {
        const std::string fn = "kz_model_int8_taps_path";
        PathPlan plan;
        int n = 0, tap_dtype = 0;
        if (int8_tap_plan(fn, model, max_batch, dtype, plan, n, tap_dtype)) return 1;
        const std::string name = path_name(plan, KZ_DTYPE_F16);
        if (!buf || len < name.size() + 1) return fail(fn + ": buffer of at least " + std::to_string(name.size() + 1) + " bytes needed");
        memcpy(buf, name.c_str(), name.size() + 1);
        return 0;
    });
}

KZ_API int kz_model_int8_taps(const kz_model *model, int device, int max_batch, int dtype, const uint8_t *bits, size_t bits_stride,
                              const float *scalars_in, int batch, int site_first, int n_sites, void *image_out_, float *stream_out) {
    return guarded("kz_model_int8_taps", [&]() -> int {
        const std::string fn = "kz_model_int8_taps";
        int8_t *image_out = static_cast<int8_t *>(image_out_);
        if (!model || !bits || (!image_out && !stream_out)) return fail(fn + ": null argument");
        PathPlan plan;
        int n = 0, tap_dtype = 0;
        if (int8_tap_plan(fn, model, max_batch, dtype, plan, n, tap_dtype)) return 1;
        if (site_first < 0 || n_sites < 1 || site_first > n - n_sites)
            return fail(fn + ": sites [" + std::to_string(site_first) + ", " + std::to_string((long long)site_first + n_sites) + ") out of range (" +
                        std::to_string(n) + " sites)");
        const Model &src = *model->m;
        if (tap_arguments(fn, src, max_batch, bits, bits_stride, scalars_in, batch)) return 1;
        EnginePtr e(nullptr, kz_engine_destroy);
        if (tap_engine(fn, model, device, max_batch, tap_dtype, Profile::taps, batch, e)) return 1;
        e->tap_geometry_batch = batch;
        // the host loop reads a site's rows strided, as the engine keeps them (the widened channels are not returned), and transposes
        const size_t hw = (size_t)src.h * src.w, ld8 = (size_t)e->tap_image_ld(), ld16 = (size_t)e->tap_stream_ld(), channels = (size_t)e->out_channels;
        std::vector<int8_t> h8((size_t)e->tap_boards * hw * ld8);
        std::vector<_Float16> h16((size_t)e->tap_boards * hw * ld16);
        for (int lo = 0; lo < batch; lo += e->tap_boards) {
            const int nb = std::min(e->tap_boards, batch - lo);
            if (tap_pass(e.get(), bits + (size_t)lo * bits_stride, bits_stride, src.n_scalar ? scalars_in + (size_t)lo * src.n_scalar : nullptr, nb))
                return fail(fn + ": " + std::string(g_err));
            const size_t rows = (size_t)nb * hw;
            for (int si = 0; si < n_sites; si++) {
                const int site = site_first + si;
                const bool has_image = site < n - 1, has_stream = site % 2 == 0;
                const size_t at = (((size_t)si * batch + lo) * channels) * hw;
                if (image_out && has_image) HIP_TRY(hipMemcpy(h8.data(), e->tap_site(site), rows * ld8, hipMemcpyDeviceToHost));
                if (stream_out && has_stream) HIP_TRY(hipMemcpy(h16.data(), e->tap_stream(site), rows * ld16 * 2, hipMemcpyDeviceToHost));
                for (size_t r = 0; r < rows; r++) {
                    const size_t o = at + (r / hw) * channels * hw + r % hw;
                    for (size_t c = 0; c < channels; c++) {
                        if (image_out) image_out[o + c * hw] = has_image ? h8[r * ld8 + c] : (int8_t)0;  // (the last site has no image)
                        if (stream_out) stream_out[o + c * hw] = has_stream ? (float)h16[r * ld16 + c] : NAN;  // (a mid site no stream)
                    }
                }
            }
        }
        return 0;
    });
}

static_assert(sizeof(kz_int8_site_error) == 120 && sizeof(kz::Int8SiteDeviation) == sizeof(kz_int8_site_error), "a device record is a kz_int8_site_error");
KZ_API int kz_model_int8_error_profile(const kz_model *model, int device, int max_batch, int dtype, const uint8_t *bits, size_t bits_stride,
                                       const float *scalars_in, int batch, void *out) {
    return guarded("kz_model_int8_error_profile", [&]() -> int {
        const std::string fn = "kz_model_int8_error_profile";
        if (!model || !bits || !out) return fail(fn + ": null argument");
        PathPlan plan;
        int n = 0, tap_dtype = 0;
        if (int8_tap_plan(fn, model, max_batch, dtype, plan, n, tap_dtype)) return 1;
        const Model &src = *model->m;
        if (tap_arguments(fn, src, max_batch, bits, bits_stride, scalars_in, batch)) return 1;
        // the references of kz_model_error_profile: the one-launch f32 tower's taps where that kernel takes the shape, else the
        // per-layer exact-f32 engine, which drives both reductions of a site as it produces it
        const bool resident = range_profile_resident(src);
        EnginePtr e(nullptr, kz_engine_destroy), ref(nullptr, kz_engine_destroy);
        if (tap_engine(fn, model, device, max_batch, tap_dtype, Profile::taps, resident ? batch : std::min(batch, 64), e)) return 1;
        e->tap_geometry_batch = batch;
        const int chunk = std::min(batch, e->tap_boards);
        if (tap_engine(fn, model, device, chunk, KZ_DTYPE_F32, resident ? Profile::taps_reference : Profile::per_layer_deviation, chunk, ref)) return 1;
        kz::Int8SiteDeviation *dev = nullptr;
        if (e->dmalloc((void **)&dev, (size_t)n * sizeof(kz::Int8SiteDeviation))) return fail(fn + ": " + std::string(g_err));
        HIP_TRY(hipMemset(dev, 0, (size_t)n * sizeof(kz::Int8SiteDeviation)));
        HIP_TRY(hipDeviceSynchronize());  // (the engines' streams do not wait for the null stream)
        if (!resident) {
            ref->tap_peer = e.get();
            ref->deviation8 = dev;
        }
        for (int lo = 0; lo < batch; lo += chunk) {
            const int nb = std::min(chunk, batch - lo);
            const uint8_t *b = bits + (size_t)lo * bits_stride;
            const float *sc = src.n_scalar ? scalars_in + (size_t)lo * src.n_scalar : nullptr;
            if (tap_pass(e.get(), b, bits_stride, sc, nb)) return fail(fn + ": " + std::string(g_err));
            if (resident) {
                if (tap_pass(ref.get(), b, bits_stride, sc, nb)) return fail(fn + ": " + std::string(g_err));
                const Pass p = ref->pass_staged(0);
                for (int site = 0; site < n; site++)
                    if (e->tap_deviation8(p, site, reinterpret_cast<const float *>(ref->tap_site(site)), ref->model->channels, nb, dev + site))
                        return fail(fn + ": " + std::string(g_err));
                HIP_TRY(hipStreamSynchronize(p.stream));
            } else {
                kz_engine::Slot &s = ref->slots[0];
                ref->stage_boards(s, b, bits_stride, sc, nb);
                const Pass p = ref->pass_staged(0);
                if (ref->copy_boards_in(p, s, nb)) return fail(fn + ": " + std::string(g_err));
                const kz::PackedBoards in = ref->packed_boards(s.d_bits, ref->bits_bytes(), s.d_sin);
                if (ref->launch(p, "kz_encode_packed", [&] { kz::launch_encode_packed(ref->dtype, in, nb, src.h * src.w, ref->x_in, ref->cin_p, p.stream); }) ||
                    ref->run_tower(p, nb, s.d_sout + kz_engine::SOUT_HDR, s.d_pol))
                    return fail(fn + ": " + std::string(g_err));
                if (ref->range_site != n) return fail(fn + ": internal error: " + std::to_string(ref->range_site) + " sites compared, " + std::to_string(n) + " expected");
                HIP_TRY(hipStreamSynchronize(p.stream));
            }
        }
        kz_int8_site_error *rec = static_cast<kz_int8_site_error *>(out);
        HIP_TRY(hipMemcpy(rec, dev, (size_t)n * sizeof(kz_int8_site_error), hipMemcpyDeviceToHost));
        for (int site = 0; site < n; site++) {
            rec[site].exponent = site < n - 1 ? e->model->i8_exp[site] : 0;
            rec[site].reserved = 0;
        }
        return 0;
    });
}

KZ_API int kz_engine_max_batch(const kz_engine *e) { return e ? e->max_batch : 0; }

KZ_API const char *kz_engine_tower_path(const kz_engine *e) { return e ? path_name(e->plan, e->dtype) : ""; }

KZ_API int kz_engine_launch_geometry(const kz_engine *e, int batch, int *workgroups, int *boards_per_workgroup) {
    return guarded("kz_engine_launch_geometry", [&]() -> int {
        if (!e || !workgroups || !boards_per_workgroup) return fail("kz_engine_launch_geometry: null argument");
        if ((batch < 0 || batch > e->max_batch ? fail("kz_engine_launch_geometry: batch out of range") : 0)) return 1;
        launch_geometry_of(*e->model, e->plan, e->dtype, batch, workgroups, boards_per_workgroup);
        return 0;
    });
}

static int check_packed(const kz_engine *e, const char *fn) {
    if (e && e->model->n_scalar < 0) return fail(no_plane_split(fn));
    return 0;
}

static int check_batch(const kz_engine *e, int batch, const char *fn) {
    if (!e) return fail(std::string(fn) + ": null engine");
    if (batch < 0 || batch > e->max_batch)  // assert!(batch_size <= max_batch_size), cudnn.rs:58
        return fail(std::string(fn) + ": batch " + std::to_string(batch) + " exceeds max_batch " +
                    std::to_string(e->max_batch));
    return 0;
}

static int slot_of(const std::string &fn, kz_engine *e, int slot, kz_engine::Slot *&s) {
    if (slot < 0 || slot >= KZ_ENGINE_SLOTS) return fail(fn + ": bad slot");
    s = &e->slots[slot];
    return 0;
}

// what both averaged entries check first: tables set, batch * n_sym within max_batch
static int check_avg(const char *name, const kz_engine *e, int batch) {
    const std::string fn = name;
    if (!e) return fail(fn + ": null engine");
    if (check_packed(e, name)) return 1;
    if (!e->n_sym) return fail(fn + ": no tables set (call kz_engine_set_symmetries first)");
#ifdef KZ_EXPERIMENTS
    if (e->plan.nb4) return fail(fn + ": the four-board experiment launch takes no symmetry ids");
#endif
    const int n = e->n_sym, limit = e->max_batch / n;
    if (batch < 0 || batch > limit)
        return fail(fn + ": batch " + std::to_string(batch) + " exceeds max_batch / n_sym = " + std::to_string(limit) + " (" +
                    std::to_string(n) + " symmetries: the network runs on batch * n_sym boards, max_batch " + std::to_string(e->max_batch) + ")");
    return 0;
}

// The host-pointer entries by what they submit (`decoded` with ids is the `_sym` entry), and what each checks first.
enum class Entry { raw, decoded, averaged };
static int check_entry(const char *fn, Entry kind, const kz_engine *e, int batch) {
    return kind == Entry::averaged ? check_avg(fn, e, batch) : check_batch(e, batch, fn) || check_packed(e, fn);
}
static int submit(const char *name, Entry kind, kz_engine *e, int slot, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                  int batch, const uint8_t *sym, const int64_t *move_offsets, const int32_t *move_indices);  // (below)

// ------------------------------------------------------------------------------------------------
// Per-board status (KZ_BOARD_*) and the range fallback: what the calls that return a batch do once its event has been waited for
// ------------------------------------------------------------------------------------------------
// The status of the boards of a finished batch `f` of slot `s`, from the per-board words the launches wrote (kz_kernels.hpp),
// into s.status: the decode's words, and the range words in front of the pinned header where they are this batch's
// (InFlight::words_in_front).
static void board_status(kz_engine::Slot &s, const InFlight &f) {
    const int *nf = reinterpret_cast<const int *>(s.h_sout);
    const bool front = f.words_in_front();
    for (int b = 0; b < f.batch; b++) {
        uint8_t st = KZ_BOARD_OK;
        if (f.is_decoded()) {
            if (s.h_err[kz::ERR_HDR + 2 * b]) st |= KZ_BOARD_BAD_DECODE;
            if (s.h_err[kz::ERR_HDR + 2 * b + 1]) st |= KZ_BOARD_NONFINITE;
        }
        if (front && nf[-1 - b] == f.epoch) st |= KZ_BOARD_NONFINITE;
        s.status[b] = st;
    }
}

// `n` boards of batch `f` in slot `s`'s pinned input staging, picked by index into one contiguous batch for a sibling's submit:
// bits, scalars and — decoded — the CSR move lists, with the symmetry ids where they travel.  The one gather of the range
// fallback and the audit.
static void gather_boards(const kz_engine *e, const kz_engine::Slot &s, const InFlight &f, const int *boards, int n, BoardGather &g) {
    const size_t bits_bytes = e->bits_bytes(), ns = (size_t)std::max(e->model->n_scalar, 0);
    g.bits.resize((size_t)n * bits_bytes);
    g.sin.resize((size_t)n * ns);
    g.sym.resize((size_t)n);
    g.moff.assign(1, 0);
    g.midx.clear();
    for (int i = 0; i < n; i++) {
        const int b = boards[i];
        memcpy(g.bits.data() + (size_t)i * bits_bytes, s.h_bits + (size_t)b * bits_bytes, bits_bytes);
        if (ns) memcpy(g.sin.data() + (size_t)i * ns, s.h_sin + (size_t)b * ns, ns * 4);
        if (!f.is_decoded()) continue;
        if (f.ids_travel()) g.sym[i] = s.h_sym[b];
        if (s.h_moff[b + 1] > s.h_moff[b]) g.midx.insert(g.midx.end(), s.h_midx + s.h_moff[b], s.h_midx + s.h_moff[b + 1]);
        g.moff.push_back((int64_t)g.midx.size());
    }
    g.midx.push_back(0);  // (never read: a non-null pointer for an empty list)
}

// A gathered batch submitted to slot `slot` of sibling `sib` as the entry that matches batch `f`'s own would: raw rows, decoded
// with the same symmetry ids (or none), or averaged.
static int submit_gathered(kz_engine *sib, int slot, const InFlight &f, int n, const BoardGather &g) {
    const Entry kind = !f.is_decoded() ? Entry::raw : f.avg ? Entry::averaged : Entry::decoded;
    const char *name = kind == Entry::raw        ? "kz_engine_submit_packed"
                       : kind == Entry::averaged ? "kz_engine_submit_packed_decoded_avg"
                                                 : "kz_engine_submit_packed_decoded_sym";
    return guarded(name, [&]() -> int {
        return submit(name, kind, sib, slot, g.bits.data(), sib->bits_bytes(), g.sin.data(), n, f.ids_travel() ? g.sym.data() : nullptr,
                      g.moff.data(), g.midx.data());
    });
}

// A sibling's slot is waited for through its event, not through the sibling's entries: its per-board verdict is what is wanted
// (in fs.status; the results stay in its pinned staging).
static int wait_sibling(kz_engine::Slot &fs) {
    const InFlight f = fs.take();
    HIP_TRY(hipEventSynchronize(fs.done));
    board_status(fs, f);
    return 0;
}

// The boards of a finished batch that carry KZ_BOARD_NONFINITE, re-evaluated through the sibling engine's matching entry (raw
// rows, decoded with the same symmetry ids, or averaged) from the slot's pinned input staging, in chunks of the sibling's
// max_batch; its results go over those boards' rows and ranges of the slot's output staging and their status becomes
// KZ_BOARD_FELL_BACK (a board still bad in exact f32 keeps its bits beside it).  Host-driven, inside the returning call.
static int range_fallback(kz_engine *e, kz_engine::Slot &s, const InFlight &f) {
    kz_engine *sib = e->fallback;
    std::vector<int> bad;
    for (int b = 0; b < f.batch; b++)
        if (s.status[b] & KZ_BOARD_NONFINITE) bad.push_back(b);
    if (bad.empty()) return 0;
    const size_t plen = (size_t)e->model->policy_len;
    const size_t per = f.avg ? (size_t)(sib->max_batch / std::max(e->n_sym, 1)) : (size_t)sib->max_batch;
    if (per < 1) return 0;  // (more symmetries than the sibling holds boards: such an averaged batch keeps its verdict)
    kz_engine::Slot &fs = sib->slots[0];
    BoardGather g;
    for (size_t lo = 0; lo < bad.size(); lo += per) {
        const int n = (int)std::min(per, bad.size() - lo);
        gather_boards(e, s, f, bad.data() + lo, n, g);
        if (submit_gathered(sib, 0, f, n, g) || wait_sibling(fs)) return 1;
        const std::vector<int64_t> &moff = g.moff;
        for (int i = 0; i < n; i++) {
            const int b = bad[lo + i];
            if (!f.is_decoded()) {
                memcpy(s.h_sout + kz_engine::SOUT_HDR + (size_t)b * 5, fs.h_sout + kz_engine::SOUT_HDR + (size_t)i * 5, 20);
                memcpy(s.h_pol + (size_t)b * plen, fs.h_pol + (size_t)i * plen, plen * 4);
            } else {
                memcpy(s.h_values + (size_t)b * 5, fs.h_values + (size_t)i * 5, 20);
                const size_t len = (size_t)(moff[i + 1] - moff[i]);
                if (len) memcpy(s.h_probs + s.h_moff[b], fs.h_probs + moff[i], len * 4);
            }
            s.status[b] = fs.status[i] ? (uint8_t)(s.status[b] | KZ_BOARD_FELL_BACK) : (uint8_t)KZ_BOARD_FELL_BACK;
        }
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The shadow audit (kz_engine_set_audit): a sample of the decoded batches, evaluated a second time by a sibling engine in a
// <= 1e-4 arithmetic and compared on the host.  Nothing of the batch itself is touched.
// ------------------------------------------------------------------------------------------------
// The tail of every decoded submit while the audit is on, once the batch's own launches and event are enqueued and before its
// record `f` goes into the slot: counts the submit and, every period-th time, hands the first k boards of the slot's input
// staging to the sibling's slot of the same index, where they run on the sibling's own stream beside the batch; f.audit_k = k.
// A failing sibling submit fails this submit with the sibling's message, and the slot stays free.
static int audit_submit(kz_engine *e, int slot, InFlight &f) {
    kz_engine::Audit &a = *e->audit;
    kz_engine::Slot &s = e->slots[slot];
    if (a.submits++ % a.period) return 0;
    int k = std::min(a.boards, f.batch);
    if (f.avg) k = std::min(k, a.sibling->max_batch / std::max(e->n_sym, 1));
    if (k < 1) return 0;
    kz_engine::Slot &fs = a.sibling->slots[slot];
    if (fs.fly.busy()) {  // (left behind by a returning call that failed before its comparison)
        (void)hipEventSynchronize(fs.done);
        fs.take();
    }
    std::vector<int> &first = a.first;
    if ((int)first.size() < k)
        for (int b = (int)first.size(); b < k; b++) first.push_back(b);
    gather_boards(e, s, f, first.data(), k, a.gather);
    if (submit_gathered(a.sibling, slot, f, k, a.gather)) {
        (void)hipEventSynchronize(s.done);  // (the batch's own launches still use the staging of the slot that stays free)
        return 1;
    }
    f.audit_k = k;
    return 0;
}

static void audit_accumulate(float engine, float sibling, float &max_abs, double &sum_sq) {
    const float d = fabsf(engine - sibling);
    max_abs = fmaxf(max_abs, d);
    sum_sq += (double)d * (double)d;
}

// The returning call's half, after the status and the fallback: waits for the sibling's slot, then compares the boards whose
// status is 0 on both sides, in batch order — the five values, then the probabilities in the caller's move order.
static int audit_compare(kz_engine *e, kz_engine::Slot &s, const InFlight &f) {
    kz_engine::Audit &a = *e->audit;
    kz_engine::Slot &fs = a.sibling->slots[&s - e->slots];
    if (wait_sibling(fs)) return 1;
    kz_audit_stats &st = a.stats;
    st.batches++;
    for (int b = 0; b < f.audit_k; b++) {
        if (s.status[b] != KZ_BOARD_OK || fs.status[b] != KZ_BOARD_OK) {
            st.skipped++;
            continue;
        }
        st.boards++;
        for (int c = 0; c < 5; c++) audit_accumulate(s.h_values[(size_t)b * 5 + c], fs.h_values[(size_t)b * 5 + c], st.max_abs_value[c], st.sum_sq_value[c]);
        // (the first k boards: the sibling's ranges start where the batch's do)
        for (int64_t i = s.h_moff[b]; i < s.h_moff[b + 1]; i++) audit_accumulate(s.h_probs[i], fs.h_probs[i], st.max_abs_prob, st.sum_sq_prob);
        st.moves += s.h_moff[b + 1] - s.h_moff[b];
    }
    return 0;
}

// What every call that returns a batch does after the slot's event, with the record it took from the slot: the per-board
// status, the fallback where it is on, and — judge = true, the entries without a status output — the verdict those entries
// have always given, with their messages.  Without a fell-back board the verdict is read from the per-batch words exactly as
// before; with one, from the boards' status (the per-batch words still hold what the replaced results raised).
static int finish_batch(const char *name, kz_engine *e, kz_engine::Slot &s, const InFlight &f, bool judge) {
    const std::string fn = name;
    board_status(s, f);
    if (e->fallback && range_fallback(e, s, f)) return 1;
    if (e->audit && f.audit_k && audit_compare(e, s, f)) return 1;
    if (!judge) return 0;
    const auto softmax_message = [&] {
        return fn + ": Softmax input sum must be strictly positive (or a move index is out of range" +
               (f.symmetries_involved() ? ", a symmetry id is not below n_sym, or a listed move has no image under its board's symmetry)" : ")");
    };
    bool fell_back = false, nonfinite = false, bad_decode = false;
    for (int b = 0; b < f.batch; b++) {
        fell_back |= (s.status[b] & KZ_BOARD_FELL_BACK) != 0;
        nonfinite |= (s.status[b] & KZ_BOARD_NONFINITE) != 0;
        bad_decode |= (s.status[b] & KZ_BOARD_BAD_DECODE) != 0;
    }
    if (fell_back) {
        if (nonfinite) return fail(kz_engine::nonfinite_message(name));
        if (bad_decode) return fail(softmax_message());
        return 0;
    }
    if (f.flag_in_header() && kz_engine::slot_nonfinite(s, f.epoch)) return fail(kz_engine::nonfinite_message(name));
    if (!f.is_decoded()) return 0;
    if (s.h_err[1]) return fail(kz_engine::nonfinite_message(name));
    if (s.h_err[0]) return fail(softmax_message());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Submit: every host-pointer entry is one body
// ------------------------------------------------------------------------------------------------
// A decoded submit's arguments (batch > 0) checked, then the boards and the CSR move lists copied into the slot's pinned
// staging (allocated and grown here); the error words cleared.
static int stage_decoded(const char *fn, kz_engine *e, kz_engine::Slot &s, const uint8_t *bits, size_t bits_stride,
                         const float *scalars_in, int batch, const int64_t *move_offsets, const int32_t *move_indices, size_t &total_out) {
    if (!bits || !move_offsets) return fail(std::string(fn) + ": null argument");
    if (bits_stride < e->bits_bytes()) return fail(std::string(fn) + ": bits_stride too small");
    if (e->model->n_scalar && !scalars_in) return fail(std::string(fn) + ": null scalars");
    if (move_offsets[0] != 0) return fail(std::string(fn) + ": move_offsets[0] must be 0");
    for (int b = 0; b < batch; b++)
        if (move_offsets[b + 1] < move_offsets[b]) return fail(std::string(fn) + ": move_offsets must be non-decreasing");
    const size_t total = (size_t)move_offsets[batch];
    if (total && !move_indices) return fail(std::string(fn) + ": null move list");
    HIP_TRY(hipSetDevice(e->device));
    if (!s.h_moff) {  // (pinned only: the decode reads and writes the host staging directly, on every path)
        if (e->hmalloc((void **)&s.h_moff, (size_t)(e->max_batch + 1) * 8) || e->hmalloc((void **)&s.h_values, (size_t)e->max_batch * 20) ||
            e->hmalloc((void **)&s.h_err, kz::error_flag_words(e->max_batch) * 4))
            return 1;
    }
    if (total > s.move_cap) {  // the old (smaller) buffers stay on the engine's free list until it is destroyed
        const size_t cap = std::max(total, std::max(s.move_cap * 2, (size_t)e->max_batch * 64));
        if (e->hmalloc((void **)&s.h_midx, cap * 4) || e->hmalloc((void **)&s.h_probs, cap * 4)) return 1;
        s.move_cap = cap;
    }
    e->stage_boards(s, bits, bits_stride, scalars_in, batch);
    memcpy(s.h_moff, move_offsets, (size_t)(batch + 1) * 8);
    if (total) memcpy(s.h_midx, move_indices, total * 4);
    memset(s.h_err, 0, kz::error_flag_words(batch) * 4);  // the per-batch words and this batch's per-board ones: cleared per submit
    total_out = total;
    return 0;
}

// The virtual batch's device scratch of a slot (kz_engine::Slot::Virtual): everything sized by max_batch at the first averaged
// submit, the two move arrays for n_sym * total moves, grown the way move_cap grows.  Every buffer stays below 2 GiB.
static int virtual_scratch(const char *fn, kz_engine *e, kz_engine::Slot &s, size_t vmoves) {
    const Model &m = *e->model;
    kz_engine::Slot::Virtual &v = s.virt;
    const size_t limit = ((size_t)1 << 31) - 1, mb = (size_t)e->max_batch, bits_bytes = e->bits_bytes();
    const auto too_large = [&](size_t bytes) {
        return bytes > limit && fail(std::string(fn) + ": a scratch buffer of the virtual batch would need " + std::to_string(bytes) +
                                     " bytes (every engine tensor must stay below 2 GiB)");
    };
    if (!v.moff) {
        const size_t ns = m.n_scalar < 0 ? 0 : (size_t)m.n_scalar;
        if (too_large(mb * bits_bytes) || too_large(mb * ns * 4) || too_large((mb + 1) * 8) || too_large(mb * 20)) return 1;
        if (e->dmalloc((void **)&v.bits, mb * bits_bytes) || e->dmalloc((void **)&v.sin, mb * ns * 4) || e->dmalloc((void **)&v.sym, mb) ||
            e->dmalloc((void **)&v.values, mb * 20) || e->dmalloc((void **)&v.err, kz::error_flag_words(e->max_batch) * 4) || e->dmalloc((void **)&v.moff, (mb + 1) * 8))
            return 1;
    }
    if (vmoves > v.move_cap) {  // the old (smaller) buffers stay on the engine's free list until it is destroyed
        const size_t cap = std::max(vmoves, std::max(v.move_cap * 2, mb * 64));
        if (too_large(cap * 4)) return 1;
        if (e->dmalloc((void **)&v.midx, cap * 4) || e->dmalloc((void **)&v.probs, cap * 4)) return 1;
        v.move_cap = cap;
    }
    return 0;
}

// kz_engine_submit_packed (raw), _decoded, _decoded_sym (decoded with sym) and _decoded_avg (averaged): the boards into the
// slot's pinned staging, one network pass on the slot's stream, the slot in flight.
//   direct ("+heads" launches, zero copy): ONE launch and no copy operation.  It reads the packed boards and the move lists
//     from the pinned staging and writes there — raw rows (136 B in, 7.5 KB out per chess board), or, decode_output
//     (common.rs:16-100) being its last step, the decoded values and the available moves' probabilities (0.2 KB per chess
//     evaluation cross PCIe; the conv policy heads keep their logits in s.d_pol for the gather, the attention network's never
//     leave LDS).
//   otherwise: the boards are copied in, the network leaves scalars and logits in device memory, and either both are copied
//     back (raw) or the stand-alone kz_decode_output reads the move lists from and writes values / probabilities / flags to
//     the pinned staging directly.
//   averaged (kz_symmetry_avg.hip): kz_sym_fan_out builds the VIRTUAL batch — every board under every symmetry, ids = k — from
//     the pinned staging in device scratch, the unchanged pass and decode run over it, kz_sym_average folds it into the
//     pinned staging.
static int submit(const char *name, Entry kind, kz_engine *e, int slot, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                  int batch, const uint8_t *sym, const int64_t *move_offsets, const int32_t *move_indices) {
    const std::string fn = name;
    const bool raw = kind == Entry::raw, avg = kind == Entry::averaged;
    if (check_entry(name, kind, e, batch)) return 1;
    if (sym && !e->n_sym) return fail(fn + ": symmetry ids given but no tables set (call kz_engine_set_symmetries first)");
#ifdef KZ_EXPERIMENTS
    if (sym && e->plan.nb4) return fail(fn + ": the four-board experiment launch takes no symmetry ids");
#endif
    kz_engine::Slot *slot_ptr = nullptr;
    if (slot_of(fn, e, slot, slot_ptr)) return 1;
    kz_engine::Slot &s = *slot_ptr;
    if (s.fly.busy()) return fail(fn + ": slot still in flight (call " + (raw ? "kz_engine_wait" : "kz_engine_wait_decoded") + " first)");
    InFlight f;  // goes into the slot whole, once the event is recorded: a failed submit leaves the slot free
    f.kind = raw ? InFlight::raw : InFlight::decoded;
    f.batch = batch;
    if (batch == 0) {
        s.fly = f;
        return 0;
    }
    const Model &m = *e->model;
    const size_t bits_bytes = e->bits_bytes();
    if (raw) {
        if (!bits || (m.n_scalar && !scalars_in)) return fail(fn + ": null input");
        if (bits_stride < bits_bytes) return fail(fn + ": bits_stride too small");
        HIP_TRY(hipSetDevice(e->device));
        e->stage_boards(s, bits, bits_stride, scalars_in, batch);
    } else {
        if (stage_decoded(name, e, s, bits, bits_stride, scalars_in, batch, move_offsets, move_indices, f.moves)) return 1;
        if (sym) memcpy(s.h_sym, sym, (size_t)batch);  // the launches read the ids from the pinned staging, like the move lists
    }
    f.avg = avg;
    f.with_sym = sym != nullptr;
    const bool direct = e->zero_copy && e->plan.heads;
    f.in_launch = direct && !raw;
#ifdef KZ_EXPERIMENTS
    const bool replayed = raw && !direct && e->graph_mode();
    const Pass p = replayed ? e->pass_replayed(slot) : direct ? e->pass_pinned(slot) : e->pass_staged(slot);
#else
    const Pass p = direct ? e->pass_pinned(slot) : e->pass_staged(slot);
#endif
    f.epoch = p.nf_epoch;
    // where the network reads `n` boards and their ids, and where the decode reads lists and writes values, probs and err:
    // the pinned staging, the device copies, or the virtual batch
    int n = batch;
    kz::PackedBoards in;
    kz::DecodeArgs dec;
    if (avg) {
        n = batch * e->n_sym;
        if (virtual_scratch(name, e, s, (size_t)e->n_sym * f.moves)) return 1;
        const kz_engine::Slot::Virtual &v = s.virt;
        const kz::SymFanOutArgs fan{s.h_bits, bits_bytes, s.h_sin, m.n_scalar, batch, e->n_sym, s.h_moff, s.h_midx,
                                    v.bits, v.sin, v.sym, v.moff, v.midx, v.err};
        if (e->launch(p, "kz_sym_fan_out", [&] { kz::launch_sym_fan_out(fan, p.stream); })) return 1;
        in = e->packed_boards(v.bits, bits_bytes, v.sin, v.sym);
        dec = kz::DecodeArgs{v.moff, v.midx, v.values, v.probs, v.err, v.sym, e->d_policy_map, e->n_sym};
    } else {
        const uint8_t *ids = sym ? s.h_sym : nullptr;
        if (!direct && e->copy_boards_in(p, s, batch)) return 1;
        in = direct ? e->packed_boards(s.h_bits, bits_bytes, s.h_sin, ids) : e->packed_boards(s.d_bits, bits_bytes, s.d_sin, ids);
        if (!raw) dec = kz::DecodeArgs{s.h_moff, s.h_midx, s.h_values, s.h_probs, s.h_err, ids, ids ? e->d_policy_map : nullptr, ids ? e->n_sym : 0};
    }
    // raw rows of a direct launch go to the pinned staging; everything else the network writes stays in device memory
    float *sout = (raw && direct ? s.h_sout : s.d_sout) + kz_engine::SOUT_HDR, *pol = raw && direct ? s.h_pol : s.d_pol;
    const auto network = [&]() -> int { return e->forward_packed(p, in, n, sout, pol, f.in_launch ? &dec : nullptr); };
#ifdef KZ_EXPERIMENTS
    if (replayed) {
        if (e->replay(p, slot, batch, s.d_bits, bits_bytes, s.d_sin, s.d_sout, s.d_pol, [&]() -> int {
                HIP_TRY(hipMemsetAsync(s.d_sout - e->front_words(), 0, ((size_t)e->front_words() + 1) * 4, p.stream));
                return network();
            }))
            return 1;
    } else
#endif
    if (network()) return 1;
#ifdef KZ_EXPERIMENTS
    if (raw && !direct) e->graph_warm = true;  // (the first pass runs eagerly: lazy per-kernel set-up must not land in a capture)
#endif
    if (raw && !direct) {
        // (one copy: the batch's per-board range words, the header, the scalars)
        HIP_TRY(hipMemcpyAsync(s.h_sout - batch, s.d_sout - batch, ((size_t)batch * 6 + kz_engine::SOUT_HDR) * 4, hipMemcpyDeviceToHost, p.stream));
        HIP_TRY(hipMemcpyAsync(s.h_pol, s.d_pol, (size_t)batch * m.policy_len * 4, hipMemcpyDeviceToHost, p.stream));
    }
    if (!raw && !direct &&
        e->launch(p, "kz_decode_output", [&] {
            kz::launch_decode_output(sout, pol, n, m.policy_len, dec.move_offsets, dec.move_indices, dec.values, dec.probs, dec.error_flag,
                                     p.nf_flag, p.nf_epoch, p.stream, dec.sym, dec.policy_map, dec.n_sym);
        }))
        return 1;
    if (avg) {
        // (a direct launch stamped its virtual boards' range words in front of the pinned header; the stand-alone decode has
        // already copied them into v.err)
        const kz::SymAverageArgs fold{dec.values, dec.probs, dec.move_offsets, dec.error_flag, batch, e->n_sym, s.h_values, s.h_probs, s.h_err,
                                      direct ? p.nf_flag : nullptr, p.nf_epoch};
        if (e->launch(p, "kz_sym_average", [&] { kz::launch_sym_average(fold, p.stream); })) return 1;
    }
    HIP_TRY(hipEventRecord(s.done, p.stream));
    if (!raw && e->audit && audit_submit(e, slot, f)) return 1;
    s.fly = f;
    return 0;
}

KZ_API int kz_engine_submit_packed(kz_engine *e, int slot, const uint8_t *bits, size_t bits_stride,
                                   const float *scalars_in, int batch) {
    return guarded("kz_engine_submit_packed", [&]() -> int {
        return submit("kz_engine_submit_packed", Entry::raw, e, slot, bits, bits_stride, scalars_in, batch, nullptr, nullptr, nullptr);
    });
}

KZ_API int kz_engine_submit_packed_decoded(kz_engine *e, int slot, const uint8_t *bits, size_t bits_stride,
                                           const float *scalars_in, int batch, const int64_t *move_offsets,
                                           const int32_t *move_indices) {
    return guarded("kz_engine_submit_packed_decoded", [&]() -> int {
        return submit("kz_engine_submit_packed_decoded", Entry::decoded, e, slot, bits, bits_stride, scalars_in, batch, nullptr, move_offsets,
                      move_indices);
    });
}

KZ_API int kz_engine_submit_packed_decoded_sym(kz_engine *e, int slot, const uint8_t *bits, size_t bits_stride,
                                               const float *scalars_in, int batch, const uint8_t *sym,
                                               const int64_t *move_offsets, const int32_t *move_indices) {
    return guarded("kz_engine_submit_packed_decoded_sym", [&]() -> int {
        return submit("kz_engine_submit_packed_decoded_sym", Entry::decoded, e, slot, bits, bits_stride, scalars_in, batch, sym, move_offsets,
                      move_indices);
    });
}

KZ_API int kz_engine_submit_packed_decoded_avg(kz_engine *e, int slot, const uint8_t *bits, size_t bits_stride,
                                               const float *scalars_in, int batch, const int64_t *move_offsets,
                                               const int32_t *move_indices) {
    return guarded("kz_engine_submit_packed_decoded_avg", [&]() -> int {
        return submit("kz_engine_submit_packed_decoded_avg", Entry::averaged, e, slot, bits, bits_stride, scalars_in, batch, nullptr,
                      move_offsets, move_indices);
    });
}

KZ_API int kz_engine_wait(kz_engine *e, int slot, float *scalars_out, float *policy_out) {
    return guarded("kz_engine_wait", [&]() -> int {
        if (!e) return fail("kz_engine_wait: null engine");
        kz_engine::Slot *sp = nullptr;
        if (slot_of("kz_engine_wait", e, slot, sp)) return 1;
        kz_engine::Slot &s = *sp;
        if (s.fly.kind != InFlight::raw) return fail("kz_engine_wait: nothing submitted on this slot");
        const InFlight f = s.take();
        if (f.batch == 0) return 0;
        if (!scalars_out || !policy_out) return fail("kz_engine_wait: null output");
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipEventSynchronize(s.done));
        const int rc = finish_batch("kz_engine_wait", e, s, f, true);
        memcpy(scalars_out, s.h_sout + kz_engine::SOUT_HDR, (size_t)f.batch * 5 * 4);
        memcpy(policy_out, s.h_pol, (size_t)f.batch * e->model->policy_len * 4);
        return rc;
    });
}

KZ_API int kz_engine_wait_view(kz_engine *e, int slot, const float **scalars_out, const float **policy_out) {
    return guarded("kz_engine_wait_view", [&]() -> int {
        if (!e) return fail("kz_engine_wait_view: null engine");
        kz_engine::Slot *sp = nullptr;
        if (slot_of("kz_engine_wait_view", e, slot, sp)) return 1;
        if (!scalars_out || !policy_out) return fail("kz_engine_wait_view: null output");
        kz_engine::Slot &s = *sp;
        if (s.fly.kind != InFlight::raw) return fail("kz_engine_wait_view: nothing submitted on this slot");
        const InFlight f = s.take();
        *scalars_out = s.h_sout + kz_engine::SOUT_HDR;
        *policy_out = s.h_pol;
        if (f.batch == 0) return 0;
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipEventSynchronize(s.done));
        return finish_batch("kz_engine_wait_view", e, s, f, true);
    });
}

KZ_API int kz_engine_eval_packed(kz_engine *e, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                                 int batch, float *scalars_out, float *policy_out) {
    return guarded("kz_engine_eval_packed", [&]() -> int {
        if (kz_engine_submit_packed(e, 0, bits, bits_stride, scalars_in, batch)) return 1;
        return kz_engine_wait(e, 0, scalars_out, policy_out);
    });
}

// The board symmetries of the game, as the two tables the launches read (include/kz_hip.h).  Validated here, so that no id
// below n_sym can send a kernel outside a plane or the policy.
KZ_API int kz_engine_set_symmetries(kz_engine *e, int n_sym, const int32_t *square_src, const int32_t *policy_map) {
    return guarded("kz_engine_set_symmetries", [&]() -> int {
        const std::string fn = "kz_engine_set_symmetries";
        if (!e || !square_src || !policy_map) return fail(fn + ": null argument");
        if (n_sym < 1 || n_sym > 255) return fail(fn + ": n_sym " + std::to_string(n_sym) + " must be in 1..255");
        const Model &m = *e->model;
        const int hw = m.h * m.w, plen = m.policy_len;
        std::vector<char> seen(hw);
        for (int s = 0; s < n_sym; s++) {
            std::fill(seen.begin(), seen.end(), 0);
            for (int q = 0; q < hw; q++) {
                const int32_t src = square_src[(size_t)s * hw + q];
                if (src < 0 || src >= hw || seen[src])
                    return fail(fn + ": square_src row " + std::to_string(s) + " is not a permutation of 0.." + std::to_string(hw - 1));
                seen[src] = 1;
            }
            for (int i = 0; i < plen; i++) {
                const int32_t to = policy_map[(size_t)s * plen + i];
                if (to < -1 || to >= plen)
                    return fail(fn + ": policy_map[" + std::to_string(s) + "][" + std::to_string(i) + "] = " + std::to_string(to) +
                                " is outside -1.." + std::to_string(plen - 1));
            }
        }
        if (e->idle(fn)) return 1;
        HIP_TRY(hipSetDevice(e->device));
        if (e->sync_all()) return 1;
        if (!e->slots[0].h_sym)
            for (auto &s : e->slots)
                if (e->hmalloc((void **)&s.h_sym, (size_t)e->max_batch)) return 1;
        if (n_sym > e->sym_cap) {  // (smaller tables stay on the engine's free list until it is destroyed)
            e->n_sym = 0;
            if (e->dmalloc((void **)&e->d_square_src, (size_t)n_sym * hw * 4) || e->dmalloc((void **)&e->d_policy_map, (size_t)n_sym * plen * 4))
                return 1;
            e->sym_cap = n_sym;
        }
        e->n_sym = 0;
        HIP_TRY(hipMemcpy(e->d_square_src, square_src, (size_t)n_sym * hw * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->d_policy_map, policy_map, (size_t)n_sym * plen * 4, hipMemcpyHostToDevice));
        e->n_sym = n_sym;
        e->h_square_src.assign(square_src, square_src + (size_t)n_sym * hw);
        e->h_policy_map.assign(policy_map, policy_map + (size_t)n_sym * plen);
        if (e->fallback && kz_engine_set_symmetries(e->fallback, n_sym, square_src, policy_map)) return 1;  // (the range fallback's sibling)
        if (e->audit && kz_engine_set_symmetries(e->audit->sibling, n_sym, square_src, policy_map)) return 1;  // (the audit's)
        return 0;
    });
}

// kz_engine_wait_decoded (status_out == nullptr: an error inside the batch fails the call) and kz_engine_wait_decoded_status
static int wait_decoded(const char *name, kz_engine *e, int slot, const float **values_out, const float **probs_out, void **status_out) {
    const std::string fn = name;
    if (!e) return fail(fn + ": null engine");
    kz_engine::Slot *sp = nullptr;
    if (slot_of(fn, e, slot, sp)) return 1;
    if (!values_out || !probs_out) return fail(fn + ": null output");
    kz_engine::Slot &s = *sp;
    if (!s.fly.is_decoded()) return fail(fn + ": nothing submitted with a move list on this slot");
    const InFlight f = s.take();
    *values_out = s.h_values;
    *probs_out = s.h_probs;
    if (status_out) *status_out = s.status.data();
    if (f.batch == 0) return 0;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipEventSynchronize(s.done));
    return finish_batch(name, e, s, f, status_out == nullptr);
}

KZ_API int kz_engine_wait_decoded(kz_engine *e, int slot, const float **values_out, const float **probs_out) {
    return guarded("kz_engine_wait_decoded", [&]() -> int { return wait_decoded("kz_engine_wait_decoded", e, slot, values_out, probs_out, nullptr); });
}

KZ_API int kz_engine_wait_decoded_status(kz_engine *e, int slot, const float **values_out, const float **probs_out, void **status_out) {
    return guarded("kz_engine_wait_decoded_status", [&]() -> int {
        if (!status_out) return fail("kz_engine_wait_decoded_status: null output");
        return wait_decoded("kz_engine_wait_decoded_status", e, slot, values_out, probs_out, status_out);
    });
}

// A sibling of `e` (the range fallback's, the audit's): the model as loaded, the same device, `dtype`, a small max_batch of its
// own, its own streams, slots and staging, and the engine's symmetry tables.
static int create_sibling(const kz_engine *e, int dtype, int max_batch, kz_engine **out) {
    const kz_model source(e->source_model);
    kz_engine *f = nullptr;
    if (kz_engine_create(&source, e->device, max_batch, dtype, &f)) return 1;
    if (e->n_sym && kz_engine_set_symmetries(f, e->n_sym, e->h_square_src.data(), e->h_policy_map.data())) {
        kz_engine_destroy(f);
        return 1;
    }
    *out = f;
    return 0;
}

KZ_API int kz_engine_set_range_fallback(kz_engine *e, int dtype) {
    return guarded("kz_engine_set_range_fallback", [&]() -> int {
        const std::string fn = "kz_engine_set_range_fallback";
        if (!e) return fail(fn + ": null engine");
        if (dtype != KZ_DTYPE_F32 && dtype != -1) return fail(fn + ": dtype must be KZ_DTYPE_F32 (on) or -1 (off), got " + std::to_string(dtype));
        if (e->dtype == KZ_DTYPE_F32 && !e->split16() && !e->bf16())
            return fail(fn + ": this engine evaluates in KZ_DTYPE_F32 already (exact f32 has no f16 range to fall back from)");
        if (e->idle(fn)) return 1;
        if (dtype == -1) {
            kz_engine_destroy(e->fallback);
            e->fallback = nullptr;
            return 0;
        }
        if (e->fallback) return 0;
        // exact f32; flagged boards go through it in chunks
        return create_sibling(e, KZ_DTYPE_F32, std::min(e->max_batch, 64), &e->fallback);
    });
}

static_assert(sizeof(kz_audit_stats) == 104, "kz_audit_stats is part of the C ABI (capi.py and hip.rs mirror its layout)");

KZ_API int kz_engine_set_audit(kz_engine *e, int dtype, int period, int boards) {
    return guarded("kz_engine_set_audit", [&]() -> int {
        const std::string fn = "kz_engine_set_audit";
        if (!e) return fail(fn + ": null engine");
        if (dtype != KZ_DTYPE_F32 && dtype != KZ_DTYPE_F32_SPLIT16 && dtype != -1)
            return fail(fn + ": dtype must be KZ_DTYPE_F32 or KZ_DTYPE_F32_SPLIT16 (on: an arithmetic within 1e-4) or -1 (off), got " +
                        std::to_string(dtype));
        if (dtype == e->public_dtype())
            return fail(fn + ": this engine evaluates in that dtype already (an audit against its own arithmetic compares nothing)");
        if (e->idle(fn)) return 1;
        if (dtype == -1) {
            if (e->audit) kz_engine_destroy(e->audit->sibling);
            delete e->audit;
            e->audit = nullptr;
            return 0;
        }
        if (period < 1) return fail(fn + ": period " + std::to_string(period) + " must be at least 1");
        const int sibling_batch = std::min(e->max_batch, 64);
        if (boards < 1 || boards > sibling_batch)
            return fail(fn + ": boards " + std::to_string(boards) + " must be in 1.." + std::to_string(sibling_batch) +
                        " (the sibling engine's max_batch)");
        const kz_model source(e->source_model);
        if (dtype == KZ_DTYPE_F32_SPLIT16 && kz_model_supports_dtype(&source, dtype) != 1)
            return fail(fn + ": this model has no KZ_DTYPE_F32_SPLIT16 kernels (kz_model_supports_dtype is 0): audit it against KZ_DTYPE_F32");
        if (!e->audit || e->audit->dtype != dtype) {
            kz_engine *f = nullptr;  // created before the old one goes
            if (create_sibling(e, dtype, sibling_batch, &f)) return 1;
            if (!e->audit) e->audit = new kz_engine::Audit();
            kz_engine_destroy(e->audit->sibling);
            e->audit->sibling = f;
            e->audit->dtype = dtype;
        }
        kz_engine::Audit &a = *e->audit;
        a.period = period;
        a.boards = boards;
        a.submits = 0;
        a.stats = kz_audit_stats{};
        return 0;
    });
}

KZ_API int kz_engine_audit_stats(kz_engine *e, void *out, int reset) {
    return guarded("kz_engine_audit_stats", [&]() -> int {
        const std::string fn = "kz_engine_audit_stats";
        if (!e) return fail(fn + ": null engine");
        if (!out) return fail(fn + ": null output");
        if (!e->audit) return fail(fn + ": the audit is off (call kz_engine_set_audit first)");
        for (const auto &s : e->slots)
            if (s.fly.audit_k) return fail(fn + ": an audited batch is in flight (wait for it first)");
        memcpy(out, &e->audit->stats, sizeof(kz_audit_stats));
        if (reset) e->audit->stats = kz_audit_stats{};
        return 0;
    });
}

// the blocking decoded entries: a submit of `kind` on slot 0 and its wait (without a status output, under kz_engine_wait_decoded's name)
static int eval_decoded(const char *name, Entry kind, kz_engine *e, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                        int batch, const uint8_t *sym, const int64_t *move_offsets, const int32_t *move_indices, float *values_out,
                        float *probs_out, void *status_out = nullptr, bool with_status = false) {
    const std::string fn = name;
    if (check_entry(name, kind, e, batch)) return 1;
    if (batch == 0) return 0;
    if (!values_out || (with_status && !status_out)) return fail(fn + ": null argument");
    if (move_offsets && move_offsets[batch] > 0 && !probs_out) return fail(fn + ": null move list");
    if (submit(name, kind, e, 0, bits, bits_stride, scalars_in, batch, sym, move_offsets, move_indices)) return 1;
    const float *values = nullptr, *probs = nullptr;
    const size_t total = e->slots[0].fly.moves;
    void *status = nullptr;
    if (wait_decoded(with_status ? name : "kz_engine_wait_decoded", e, 0, &values, &probs, with_status ? &status : nullptr)) return 1;
    memcpy(values_out, values, (size_t)batch * 20);
    if (total) memcpy(probs_out, probs, total * 4);
    if (with_status) memcpy(status_out, status, (size_t)batch);
    return 0;
}

KZ_API int kz_engine_eval_packed_decoded_status(kz_engine *e, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                                                int batch, const uint8_t *sym, const int64_t *move_offsets,
                                                const int32_t *move_indices, float *values_out, float *probs_out, void *status_out) {
    return guarded("kz_engine_eval_packed_decoded_status", [&]() -> int {
        return eval_decoded("kz_engine_eval_packed_decoded_status", Entry::decoded, e, bits, bits_stride, scalars_in, batch, sym, move_offsets,
                            move_indices, values_out, probs_out, status_out, true);
    });
}

KZ_API int kz_engine_eval_packed_decoded(kz_engine *e, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                                         int batch, const int64_t *move_offsets, const int32_t *move_indices,
                                         float *values_out, float *probs_out) {
    return guarded("kz_engine_eval_packed_decoded", [&]() -> int {
        return eval_decoded("kz_engine_eval_packed_decoded", Entry::decoded, e, bits, bits_stride, scalars_in, batch, nullptr, move_offsets, move_indices,
                            values_out, probs_out);
    });
}

KZ_API int kz_engine_eval_packed_decoded_sym(kz_engine *e, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                                             int batch, const uint8_t *sym, const int64_t *move_offsets,
                                             const int32_t *move_indices, float *values_out, float *probs_out) {
    return guarded("kz_engine_eval_packed_decoded_sym", [&]() -> int {
        return eval_decoded("kz_engine_eval_packed_decoded_sym", Entry::decoded, e, bits, bits_stride, scalars_in, batch, sym, move_offsets,
                            move_indices, values_out, probs_out);
    });
}

KZ_API int kz_engine_eval_packed_decoded_avg(kz_engine *e, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                                             int batch, const int64_t *move_offsets, const int32_t *move_indices,
                                             float *values_out, float *probs_out) {
    return guarded("kz_engine_eval_packed_decoded_avg", [&]() -> int {
        return eval_decoded("kz_engine_eval_packed_decoded_avg", Entry::averaged, e, bits, bits_stride, scalars_in, batch, nullptr,
                            move_offsets, move_indices, values_out, probs_out);
    });
}

KZ_API int kz_engine_eval_dense(kz_engine *e, const float *input_nchw, int batch, float *scalars_out,
                                float *policy_out) {
    return guarded("kz_engine_eval_dense", [&]() -> int {
        if (check_batch(e, batch, "kz_engine_eval_dense")) return 1;
        if (batch == 0) return 0;
        if (!input_nchw || !scalars_out || !policy_out) return fail("kz_engine_eval_dense: null argument");
        kz_engine::Slot &s = e->slots[0];
        if (s.fly.busy()) return fail("kz_engine_eval_dense: slot 0 still in flight");
        const Model &m = *e->model;
        HIP_TRY(hipSetDevice(e->device));
        const size_t per = (size_t)m.c_in * m.h * m.w * 4;
        if (!e->d_dense) {
            if (e->dmalloc((void **)&e->d_dense, e->max_batch * per) || e->hmalloc((void **)&e->h_dense, e->max_batch * per))
                return 1;
        }
        memcpy(e->h_dense, input_nchw, batch * per);
        const Pass p = e->pass_staged(0);
        HIP_TRY(hipMemcpyAsync(e->d_dense, e->h_dense, batch * per, hipMemcpyHostToDevice, p.stream));
        if (e->forward_dense(p, e->d_dense, batch, s.d_sout + kz_engine::SOUT_HDR, s.d_pol)) return 1;
        HIP_TRY(hipMemcpyAsync(s.h_sout, s.d_sout, ((size_t)batch * 5 + kz_engine::SOUT_HDR) * 4, hipMemcpyDeviceToHost, p.stream));
        HIP_TRY(hipMemcpyAsync(s.h_pol, s.d_pol, (size_t)batch * m.policy_len * 4, hipMemcpyDeviceToHost, p.stream));
        HIP_TRY(hipStreamSynchronize(p.stream));
        memcpy(scalars_out, s.h_sout + kz_engine::SOUT_HDR, (size_t)batch * 5 * 4);
        memcpy(policy_out, s.h_pol, (size_t)batch * m.policy_len * 4);
        if (kz_engine::slot_nonfinite(s, p.nf_epoch)) return fail(kz_engine::nonfinite_message("kz_engine_eval_dense"));
        return 0;
    });
}

KZ_API int kz_engine_enqueue_packed_device(kz_engine *e, const void *d_bits, size_t bits_stride,
                                           const void *d_scalars_in, int batch, void *d_scalars_out,
                                           void *d_policy_out) {
    return guarded("kz_engine_enqueue_packed_device", [&]() -> int {
        if (check_batch(e, batch, "kz_engine_enqueue_packed_device") || check_packed(e, "kz_engine_enqueue_packed_device"))
            return 1;
        if (batch == 0) return 0;
        if (!d_bits || !d_scalars_out || !d_policy_out) return fail("kz_engine_enqueue_packed_device: null argument");
        if (bits_stride < e->bits_bytes()) return fail("kz_engine_enqueue_packed_device: bits_stride too small");
        HIP_TRY(hipSetDevice(e->device));
        const kz::PackedBoards in = e->packed_boards(d_bits, bits_stride, d_scalars_in);
    #ifdef KZ_EXPERIMENTS
        if (e->graph_mode()) {
            const Pass p = e->pass_replayed(-1);
            return e->replay(p, -1, batch, d_bits, bits_stride, d_scalars_in, d_scalars_out, d_policy_out,
                             [&]() -> int { return e->forward_packed(p, in, batch, d_scalars_out, d_policy_out); });
        }
        e->graph_warm = true;
    #endif
        return e->forward_packed(e->pass_resident(), in, batch, d_scalars_out, d_policy_out);
    });
}

KZ_API int kz_engine_enqueue_dense_device(kz_engine *e, const void *d_input_nchw, int batch, void *d_scalars_out,
                                          void *d_policy_out) {
    return guarded("kz_engine_enqueue_dense_device", [&]() -> int {
        if (check_batch(e, batch, "kz_engine_enqueue_dense_device")) return 1;
        if (batch == 0) return 0;
        if (!d_input_nchw || !d_scalars_out || !d_policy_out) return fail("kz_engine_enqueue_dense_device: null argument");
        HIP_TRY(hipSetDevice(e->device));
        return e->forward_dense(e->pass_resident(), d_input_nchw, batch, d_scalars_out, d_policy_out);
    });
}

KZ_API int kz_engine_synchronize(kz_engine *e) {
    return guarded("kz_engine_synchronize", [&]() -> int {
        if (!e) return fail("kz_engine_synchronize: null engine");
        HIP_TRY(hipSetDevice(e->device));
        if (e->sync_all()) return 1;
        return e->check_devflag();
    });
}

KZ_API int kz_device_malloc(int device, size_t bytes, void **out) {
    return guarded("kz_device_malloc", [&]() -> int {
        if (!out) return fail("kz_device_malloc: null argument");
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipMalloc(out, bytes ? bytes : 16));
        return 0;
    });
}

KZ_API int kz_device_free(int device, void *ptr) {
    return guarded("kz_device_free", [&]() -> int {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipFree(ptr));
        return 0;
    });
}

KZ_API int kz_memcpy_h2d(int device, void *dst, const void *src, size_t bytes) {
    return guarded("kz_memcpy_h2d", [&]() -> int {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        return 0;
    });
}

KZ_API int kz_memcpy_d2h(int device, void *dst, const void *src, size_t bytes) {
    return guarded("kz_memcpy_d2h", [&]() -> int {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        return 0;
    });
}

KZ_API int kz_device_synchronize(int device) {
    return guarded("kz_device_synchronize", [&]() -> int {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipDeviceSynchronize());
        return 0;
    });
}

KZ_API int kz_engine_set_profiling(kz_engine *e, int enable) {
    return guarded("kz_engine_set_profiling", [&]() -> int {
        if (!e) return fail("kz_engine_set_profiling: null engine");
        HIP_TRY(hipSetDevice(e->device));
        if (e->sync_all()) return 1;
        e->prof.clear();
        e->prof.on = enable != 0;
        return 0;
    });
}

KZ_API int kz_engine_kernel_time(kz_engine *e, const char *prefix, double *total_ms, int64_t *launches) {
    return guarded("kz_engine_kernel_time", [&]() -> int {
        if (!e || !prefix || !total_ms || !launches) return fail("kz_engine_kernel_time: null argument");
        HIP_TRY(hipSetDevice(e->device));
        if (e->sync_all()) return 1;
        double total = 0;
        int64_t n = 0;
        const size_t plen = strlen(prefix);
        for (auto &r : e->prof.recs) {
            if (r.name.compare(0, plen, prefix) != 0) continue;
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
            total += ms;
            n++;
        }
        *total_ms = total;
        *launches = n;
        return 0;
    });
}

KZ_API int kz_engine_read_activation(kz_engine *e, const char *name, int batch, float *out_nchw) {
    return guarded("kz_engine_read_activation", [&]() -> int {
        if (!e || !name || !out_nchw) return fail("kz_engine_read_activation: null argument");
        // "tower.out": the tower output of the last evaluation, on every path that materialises it (all but the fused-heads
        // launch)
        const bool tower_out = std::string(name) == "tower.out" && !e->plan.heads;
        if (!e->plan.keep && !tower_out)
            return fail("kz_engine_read_activation: engine keeps no activations (create it with KZ_FORCE_GENERIC=1 and "
                        "KZ_KEEP_ACTIVATIONS=1; \"tower.out\" is available on every path without fused heads)");
        auto it = e->kept.find(name);
        if (!tower_out && it == e->kept.end())
            return fail(std::string("kz_engine_read_activation: no activation named '") + name + "'");
        const void *src_act = tower_out ? e->act[e->tower_out] : it->second;
        if (check_batch(e, batch, "kz_engine_read_activation")) return 1;
        const Model &m = *e->model;
        const int hw = m.h * m.w, C = e->out_channels, cp = e->cp;
        HIP_TRY(hipSetDevice(e->device));
        if (e->sync_all()) return 1;
        std::vector<uint8_t> raw((size_t)batch * hw * cp * e->esz);
        HIP_TRY(hipMemcpy(raw.data(), src_act, raw.size(), hipMemcpyDeviceToHost));
        for (int b = 0; b < batch; b++)
            for (int c = 0; c < C; c++)
                for (int p = 0; p < hw; p++) {
                    const size_t src = ((size_t)b * hw + p) * cp + c;
                    float v;
                    if (e->dtype == KZ_DTYPE_F32) {
                        memcpy(&v, raw.data() + src * 4, 4);
                    } else {
                        _Float16 h;
                        memcpy(&h, raw.data() + src * 2, 2);
                        v = (float)h;
                    }
                    out_nchw[((size_t)b * C + c) * hw + p] = v;
                }
        return 0;
    });
}

}  // extern "C"
