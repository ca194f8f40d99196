// kz_engine_state.hpp — what an engine IS: the per-launch profiler, the model handle, and `struct kz_engine` with its
// path (one PathPlan of kz_plan.hpp, asked whenever a kernel choice depends on it), streams, slots (pinned staging + device
// buffers + the one InFlight record), range-check epochs, the Pass a forward pass is given, and allocation bookkeeping.  The forward pass over
// that state — which kernels run, in which order — is declared here and defined in kz_engine_forward.hpp; the `extern "C"`
// entry points that drive both are kz_engine.hip.  Included ONCE, by kz_engine.hip, inside its anonymous namespace (the
// first part) — the same arrangement as kz_engine_util.hpp / kz_plan.hpp / kz_device_weights.hpp.
#pragma once

struct Prof {
    struct Rec {
        std::string name;
        hipEvent_t a, b;
    };
    bool on = false;
    std::vector<Rec> recs;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    void clear() {
        for (auto &r : recs) pool.push_back({r.a, r.b});
        recs.clear();
    }
    void destroy() {
        clear();
        for (auto &p : pool) {
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
        pool.clear();
    }
    void begin(const char *name, hipStream_t s) {
        if (!on) return;
        Rec r;
        r.name = name;
        if (!pool.empty()) {
            r.a = pool.back().first;
            r.b = pool.back().second;
            pool.pop_back();
        } else {
            (void)hipEventCreate(&r.a);
            (void)hipEventCreate(&r.b);
        }
        (void)hipEventRecord(r.a, s);
        recs.push_back(r);
    }
    void end(hipStream_t s) {
        if (!on) return;
        (void)hipEventRecord(recs.back().b, s);
    }
};


}  // namespace

struct kz_model {
    std::shared_ptr<Model> m;
    // the tower widened to a multiple of 64 channels by zero filters (kz::pad_channels), built at first use; null when the
    // channel count is one already
    mutable std::mutex widened_mutex;
    mutable std::shared_ptr<Model> widened;
    mutable bool widened_tried = false;
    explicit kz_model(std::shared_ptr<Model> model) : m(std::move(model)) {}
};

namespace {
// The network the kernels of `dtype` run: the model itself, or — f16 / split arithmetic, a tower of 48, 96, 160 ...
// channels — the same network widened to the next multiple of 64 channels: zero filters cost (Cpad / C)^2 of the
// multiply-adds and buy the one-launch and board-tile kernels instead of the generic implicit GEMM (chess x 96 channels,
// f16: 0.53M -> 1.0M evals/s; x 160: 0.24M -> 0.6M).  Exact f32 keeps its implicit GEMM (the f32 one-launch tower exists
// for 128 / 256 channels only and the f32 matrix rate makes the zero work expensive).
std::shared_ptr<Model> effective_model(const kz_model *model, int dtype_in, int max_batch) {
    const Model &m = *model->m;
    // (the int8 arithmetic reads none of the switches: it has one tower, and that tower wants a multiple of 64 channels)
    const bool switched = !int8_dtype(dtype_in) && (env_on("KZ_FORCE_GENERIC") || env_on("KZ_KEEP_ACTIVATIONS"));
    if (dtype_in == KZ_DTYPE_F32 || m.tower_kind != kz::TOWER_RES || m.channels % 64 == 0 || m.channels > 512 || m.depth < 1 || switched)
        return model->m;
    std::shared_ptr<Model> wide;
    {
        std::lock_guard<std::mutex> lock(model->widened_mutex);
        if (!model->widened_tried) {
            model->widened_tried = true;
            model->widened.reset(kz::pad_channels(m, round_up(m.channels, 64)));
        }
        wide = model->widened;
    }
    if (!wide) return model->m;
    // The zero filters only pay when they buy another kernel: a widened tower that still takes the generic implicit GEMM
    // (Go 19x19 x 96 channels at max_batch 8: too few workgroups for the board-tile kernel) would run (Cpad / C)^2 of the
    // multiply-adds through the same kernel.  Keep the network as it is then — unless it is refused as it is (split16).
    PathPlan pw, po;
    std::string why;
    if (!plan_path(*wide, max_batch, dtype_in, pw, why)) return model->m;
    if (pw.tower == Tower::conv_igemm && plan_path(m, max_batch, dtype_in, po, why)) return model->m;
    return wide;
}
}  // namespace

// Boards of a slot's pinned input staging picked out as one contiguous batch for a sibling engine's submit: bits, scalars,
// symmetry ids and (decoded) the CSR move lists.  The range fallback gathers the flagged boards, the audit the sampled ones.
struct BoardGather {
    std::vector<uint8_t> bits, sym;
    std::vector<float> sin;
    std::vector<int64_t> moff;
    std::vector<int32_t> midx;
};

// Where a forward pass is enqueued and where its range check reports (kz::ScalarHeadArgs: a kernel that meets a non-finite
// activation raises *nf_flag to nf_epoch, and the per-board word in front of it).  Made by kz_engine's pass_* methods, one per
// origin, and handed down through forward_* / run_tower / run_heads / conv / launch / stash: nothing else says where a pass goes.
struct Pass {
    hipStream_t stream;
    int *nf_flag;
    int nf_epoch;
};

// What a slot has in flight.  ONE record: assigned whole by the submit once its event is recorded (a submit that fails
// leaves the slot free), and handed whole to the call that returns the batch by Slot::take(), which frees the slot.
struct InFlight {
    enum Kind : uint8_t { none, raw, decoded } kind = none;  // raw: scalars and policy rows; decoded: submitted with a move list
    int batch = 0;
    bool in_launch = false;  // decoded by the network's own launch ("+heads", zero copy), not by a kz_decode_output behind it
    bool avg = false;        // an averaged submit: the network ran on batch * n_sym virtual boards
    bool with_sym = false;   // the caller gave symmetry ids
    size_t moves = 0;        // decoded: move_offsets[batch]
    int audit_k = 0;         // the first audit_k boards also run on the audit's sibling (same slot index)
    int epoch = 0;           // what the range words read where this batch met a non-finite activation (Pass::nf_epoch)
    bool busy() const { return kind != none; }
    bool is_decoded() const { return kind == decoded; }
    // the per-batch range word of this batch is the pinned header's: the raw rows come with that header, and a decode inside
    // the launch leaves the word where the launch reported (pass_pinned); a stand-alone decode copies it into h_err[1]
    bool flag_in_header() const { return kind == raw || in_launch; }
    // ... and so are the per-board words in front of it — but an averaged launch's count VIRTUAL boards, which
    // kz_sym_average has folded into the decode's words like kz_decode_output does on the other paths
    bool words_in_front() const { return kind == raw || (in_launch && !avg); }
    // a sibling's submit of boards of this batch carries their ids (an averaged batch makes its own: 0 .. n_sym-1 per board)
    bool ids_travel() const { return with_sym && !avg; }
    // a decode error of this batch may be a symmetry's (an id not below n_sym, a move without an image): the error's wording
    bool symmetries_involved() const { return with_sym || avg; }
};

// bytes of one board's packed bool planes
inline size_t bits_bytes(const Model &m) { return (size_t)(m.n_bool * m.h * m.w + 7) / 8; }

struct kz_engine {
    std::shared_ptr<Model> model;
    std::shared_ptr<DeviceWeights> wts;
    int device = 0, dtype = 0, max_batch = 0;
    int out_channels = 0;  // the network's own tower channels (model->channels may be widened: effective_model)
    size_t esz = 4;
    size_t bits_bytes() const { return ::bits_bytes(*model); }
    // [0] = the main stream.  On the fused path (one launch per batch, which touches nothing but its slot's buffers) slots
    // alternate over TWO streams — a batch of 256 is half a chip of workgroups, so two launches run side by side and the
    // next launch of a stream starts the moment the previous one ends — and the launch reads the packed boards from and
    // writes the results to the slot's pinned host staging directly (zero copy): no H2D/D2H operation sits between two
    // launches of a stream.  Otherwise all slots share the main stream and staging is copied.
    hipStream_t slot_stream[KZ_ENGINE_SLOTS] = {};
    bool zero_copy = false;
    int sync_all() {
        for (auto st : slot_stream)
            if (st) HIP_TRY(hipStreamSynchronize(st));
        return 0;
    }
    std::vector<void *> allocs, pinned;
    PathPlan plan;  // which kernels run the network (plan_path, then the experiment build's switches)
    bool split16() const { return split_arithmetic(plan); }
    bool bf16() const { return plan.tower == Tower::resident_bf16g; }
    bool i8() const { return plan.tower == Tower::resident_i8 || plan.tower == Tower::board_conv_i8; }
    // the dtype kz_engine_create was given (`dtype` is KZ_DTYPE_F32 for the two f32 engines with an exchanged tower, and
    // KZ_DTYPE_F16 for the int8 engines, 4 and 5: the f16 engine with it exchanged — which of the two the plan does not say
    // where 5 plans as 4 does, so the engine keeps the value it was created with)
    int created_dtype = 0;
    int public_dtype() const { return bf16() ? KZ_DTYPE_BF16 : split16() ? KZ_DTYPE_F32_SPLIT16 : i8() ? created_dtype : dtype; }
    void *xres = nullptr;  // (experiment build, PathPlan::nb4: the four-board launch's residual scratch)

    // activations
    int cin_p = 0, cp = 0;
    void *x_in = nullptr;
    void *act[3] = {nullptr, nullptr, nullptr};
    void *act8[2] = {nullptr, nullptr};  // board_conv_i8: the int8 images X8 and Y8 beside the f16 stream, [rows][C8] bytes each
    void *head0 = nullptr, *head1 = nullptr;  // head temporaries
    int tower_out = 0;

    // host-pointer entry points: per-slot device io + pinned staging
    struct Slot {
        uint8_t *d_bits = nullptr, *h_bits = nullptr;
        float *d_sin = nullptr, *h_sin = nullptr;
        // d_sout / h_sout start with a 16-byte header: [0] = the range-check flag (kz::ScalarHeadArgs::nonfinite_flag),
        // so that it crosses PCIe in the same copy as the scalars.  IN FRONT of the header lie the range check's per-board
        // words (kz_kernels.hpp "per-board status words": board b's at [-1 - b], front_words() of them in both buffers,
        // epoch-stamped like the flag), so the copy that fetches a batch starts `batch` words earlier
        float *d_sout = nullptr, *h_sout = nullptr;
        float *d_pol = nullptr, *h_pol = nullptr;
        hipEvent_t done = nullptr;
        InFlight fly;  // what `done` stands for; kind none: the slot is free
        InFlight take() {
            const InFlight f = fly;
            fly = InFlight();
            return f;
        }
        // device-side decode (N2): CSR move lists, decoded values, probabilities, error flag; grown on demand
        size_t move_cap = 0;
        int64_t *h_moff = nullptr;
        int32_t *h_midx = nullptr;
        float *h_values = nullptr, *h_probs = nullptr;
        int *h_err = nullptr;  // [0] softmax sum / move index, [1] range check, then two words per board (kz_kernels.hpp:
                               // launch_decode_output, error_flag_words(max_batch)); cleared per submit by stage_decoded
        std::vector<uint8_t> status;  // [max_batch] KZ_BOARD_* of the batch last waited for (kz_engine_wait_decoded_status's view)
        uint8_t *h_sym = nullptr;  // [max_batch] symmetry ids of the batch (pinned, read by the launches; set_symmetries allocates it)
        // every board under every symmetry (the `_avg` entries, kz_symmetry_avg.hip): the VIRTUAL batch in device memory —
        // what kz_sym_fan_out writes and the network reads, what the decode writes and kz_sym_average reads.  Allocated at
        // the slot's first averaged submit, for max_batch virtual boards; the two move arrays grow like move_cap
        struct Virtual {
            uint8_t *bits = nullptr, *sym = nullptr;  // [max_batch][bits_bytes], [max_batch] ids
            float *sin = nullptr, *values = nullptr;  // [max_batch][n_scalar], [max_batch][5]
            int64_t *moff = nullptr;                  // [max_batch + 1]
            int *err = nullptr;                       // the decode's flag words (error_flag_words(max_batch))
            int32_t *midx = nullptr;                  // [move_cap]
            float *probs = nullptr;                   // [move_cap]
            size_t move_cap = 0;
        } virt;
    } slots[KZ_ENGINE_SLOTS];
    // board symmetries (kz_engine_set_symmetries): the two tables the encode and the decode read, in device memory
    int n_sym = 0, sym_cap = 0;
    int32_t *d_square_src = nullptr, *d_policy_map = nullptr;  // [n_sym][h*w], [n_sym][policy_len]
    std::vector<int32_t> h_square_src, h_policy_map;          // the same tables as the caller gave them (for a sibling created later)
    // the range fallback (kz_engine_set_range_fallback): a sibling engine of the same model and device in exact f32 with a
    // small max_batch of its own; the call that returns a batch re-evaluates the boards whose range word fired through it
    // (kz_engine.hip: range_fallback).  It has its own streams, slots and staging; only DeviceWeights' cache is shared.
    std::shared_ptr<Model> source_model;  // the model as loaded (`model` may be the widened one)
    kz_engine *fallback = nullptr;
    // the shadow audit (kz_engine_set_audit): a SECOND sibling, in a <= 1e-4 arithmetic, that evaluates the first boards of every
    // period-th decoded submit on its own stream beside the batch; the call that returns the batch compares the two on the host
    // and accumulates the deviation (kz_engine.hip: audit_submit, audit_compare).  Null while the audit is off: the one test the
    // decoded submits and finish_batch pay for it.
    struct Audit {
        kz_engine *sibling = nullptr;
        int dtype = -1, period = 1, boards = 1;
        int64_t submits = 0;  // decoded submits with batch > 0 since kz_engine_set_audit
        kz_audit_stats stats{};
        BoardGather gather;      // (kept between submits: no allocation per audited batch)
        std::vector<int> first;  // 0, 1, 2 ...: the sampled boards' indices, as the gather takes them
    };
    Audit *audit = nullptr;
    // words in front of every range-check flag word the engine hands to a launch (a multiple of 4: the scalars stay 16-byte aligned)
    int front_words() const { return (max_batch + 3) / 4 * 4; }
    float *d_dense = nullptr, *h_dense = nullptr;
    static constexpr int SOUT_HDR = 4;  // floats in front of the scalars
    // range check (see kz::ScalarHeadArgs): every submission gets a new epoch; a kernel that meets a non-finite
    // activation raises the flag it was given to that epoch.  No reset between batches is needed.
    // Epochs run 1 .. GRAPH_EPOCH-1 and start over (0 is the cleared word, GRAPH_EPOCH the replayed passes' constant):
    // at ~2k submissions/s an int would overflow after 12 days of self-play.
    int epoch = 0;
    int *d_devflag = nullptr;  // flag of the device-resident entry points, checked by kz_engine_synchronize
    int dev_epoch_enqueued = 0;  // epoch of the last device-resident enqueue (slot submissions do not touch d_devflag)
    int dev_epoch_checked = 0;
    int next_epoch() {
        if (epoch >= GRAPH_EPOCH - 1) {  // start over: settle the device-resident flag first (slot flags compare for equality)
            (void)sync_all();
            check_devflag_pending();
            if (d_devflag) (void)hipMemset(d_devflag - front_words(), 0, ((size_t)front_words() + 1) * 4);
            // the slots' own flag words too: a slot that once recorded a non-finite batch at epoch X keeps X in its header,
            // and X is about to be issued again (everything is idle here: sync_all above)
            for (auto &s : slots) {
                if (s.fly.busy()) continue;  // (a finished batch nobody has waited for yet keeps its verdict)
                // (with their per-board words in front: epoch-stamped like the flag itself)
                if (s.d_sout) (void)hipMemset(s.d_sout - front_words(), 0, ((size_t)front_words() + 1) * 4);
                if (s.h_sout) memset(s.h_sout - front_words(), 0, ((size_t)front_words() + 1) * 4);
            }
            epoch = dev_epoch_enqueued = dev_epoch_checked = 0;
        }
        return ++epoch;
    }
    bool wrap_nonfinite_pending = false;  // a non-finite batch seen while starting the epochs over: reported by the next synchronize
    void check_devflag_pending() {
        if (!d_devflag || dev_epoch_checked == dev_epoch_enqueued) return;
        int v = 0;
        if (hipMemcpy(&v, d_devflag, 4, hipMemcpyDeviceToHost) == hipSuccess && v != GRAPH_EPOCH && v > dev_epoch_checked)
            wrap_nonfinite_pending = true;
    }
    // ---- the passes, by origin.  A slot's pass runs on the slot's stream: its own on the fused path, so that two submitted
    // batches run side by side; otherwise the slots share the activation buffers and the main stream ----
    hipStream_t stream_of(int slot) const { return slot_stream[slot] ? slot_stream[slot] : slot_stream[0]; }
    // a slot whose results are copied back: the flag is the device header's, fetched with the scalars (or read by kz_decode_output)
    Pass pass_staged(int slot) { return Pass{stream_of(slot), reinterpret_cast<int *>(slots[slot].d_sout), next_epoch()}; }
    // a slot whose launch writes its pinned staging itself (zero copy): the flag is the pinned header's
    Pass pass_pinned(int slot) { return Pass{stream_of(slot), reinterpret_cast<int *>(slots[slot].h_sout), next_epoch()}; }
    // the device-resident entry points: the main stream, the flag kz_engine_synchronize checks
    Pass pass_resident() {
        dev_epoch_enqueued = next_epoch();
        return Pass{slot_stream[0], d_devflag, dev_epoch_enqueued};
    }

    // hipGraph replay of the forward pass (KZ_HIP_GRAPH=1; multi-launch paths only — the one-launch paths have nothing to
    // replay): the launches of one (entry point, batch size, buffers) are captured once from the engine's own stream and
    // replayed with one hipGraphLaunch.  A captured kernel argument cannot change, so the range check of a replayed pass
    // reports a CONSTANT epoch: per slot the flag word is cleared by a captured memset, for the device-resident entry
    // points kz_engine_synchronize clears it after reporting.
    static constexpr int GRAPH_EPOCH = 0x7fffffff;
#ifndef KZ_EXPERIMENTS
    static constexpr bool graph_mode() { return false; }  // the replay is an experiment build's switch (no gain measured)
#else
    bool graph_warm = false;
    struct GraphEntry {
        int kind, batch;  // kind: slot index, or -1 for the device-resident entry point
        const void *bits;
        size_t stride;
        const void *sin;
        void *sout, *pol;
        hipGraphExec_t exec;
    };
    std::vector<GraphEntry> graphs;
    bool graph_mode() const { return plan.graph && graph_warm && !prof.on && !plan.keep; }
    // a replayed pass: slot `kind`'s device header, or (-1) the device-resident flag with its enqueue noted, at the constant epoch
    Pass pass_replayed(int kind) {
        if (kind < 0) dev_epoch_enqueued = next_epoch();
        return Pass{kind < 0 ? slot_stream[0] : stream_of(kind), kind < 0 ? d_devflag : reinterpret_cast<int *>(slots[kind].d_sout), GRAPH_EPOCH};
    }
    // runs `body` (which enqueues on p.stream) through the graph of this key: captured at first sight
    template <class Body>
    int replay(const Pass &p, int kind, int batch, const void *bits, size_t stride, const void *sin, void *sout, void *pol, Body body) {
        hipStream_t stream = p.stream;
        for (const GraphEntry &g : graphs)
            if (g.kind == kind && g.batch == batch && g.bits == bits && g.stride == stride && g.sin == sin && g.sout == sout &&
                g.pol == pol) {
                HIP_TRY(hipGraphLaunch(g.exec, stream));
                return 0;
            }
        if (graphs.size() >= 32) return body();  // (a caller cycling through many shapes: eager)
        hipGraph_t graph = nullptr;
        HIP_TRY(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        const int rc = body();
        const hipError_t end = hipStreamEndCapture(stream, &graph);
        if (rc || end != hipSuccess) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc ? rc : fail(std::string("hipStreamEndCapture: ") + hipGetErrorString(end));
        }
        hipGraphExec_t exec = nullptr;
        const hipError_t inst = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (inst != hipSuccess) return fail(std::string("hipGraphInstantiate: ") + hipGetErrorString(inst));
        graphs.push_back({kind, batch, bits, stride, sin, sout, pol, exec});
        HIP_TRY(hipGraphLaunch(exec, stream));
        return 0;
    }
#endif
    static bool slot_nonfinite(const Slot &s, int epoch) { return *reinterpret_cast<const int *>(s.h_sout) == epoch; }
    // "a batch is in flight": what the calls that change something every slot depends on ask first
    int idle(const std::string &fn) const {
        for (const auto &s : slots)
            if (s.fly.busy()) return fail(fn + ": a batch is in flight (wait for every slot first)");
        return 0;
    }
    int check_devflag() {
        if (wrap_nonfinite_pending) {
            wrap_nonfinite_pending = false;
            return fail(nonfinite_message("kz_engine_synchronize"));
        }
        // nothing device-resident enqueued since the last check: no blocking copy (slot submissions report per slot)
        if (!d_devflag || dev_epoch_checked == dev_epoch_enqueued) return 0;
        int v = 0;
        HIP_TRY(hipMemcpy(&v, d_devflag, 4, hipMemcpyDeviceToHost));
        const int since = dev_epoch_checked;
        dev_epoch_checked = dev_epoch_enqueued;
        if (v == GRAPH_EPOCH) HIP_TRY(hipMemset(d_devflag, 0, 4));  // (a replayed pass cannot carry a fresh epoch)
        if (v > since) return fail(nonfinite_message("kz_engine_synchronize"));
        return 0;
    }
    static std::string nonfinite_message(const char *fn) {
        return std::string(fn) + ": non-finite activation in the network output of this batch (beyond +-65504 the f16 "
               "and split-f16 paths overflow: evaluate this network with KZ_DTYPE_F32).  kz_engine_set_range_fallback(engine, "
               "KZ_DTYPE_F32) makes the engine re-evaluate just the out-of-range boards in exact f32 instead of failing the batch";
    }

    // debugging (PathPlan::keep)
    std::map<std::string, void *> kept;

    Prof prof;

    int dmalloc(void **p, size_t bytes) {
        HIP_TRY(hipMalloc(p, bytes ? bytes : 16));
        allocs.push_back(*p);
        return 0;
    }
    int hmalloc(void **p, size_t bytes) {
        HIP_TRY(hipHostMalloc(p, bytes ? bytes : 16, hipHostMallocDefault));
        pinned.push_back(*p);
        return 0;
    }

    // the range profile (kz_model_range_profile): a profiling engine — exact f32 on the per-layer path, plan.keep set — takes
    // max |x| per board at every site where run_tower stashes, instead of the copy: range_out [n_sites][max_batch] in device
    // memory, range_site counts the sites of the running pass in stash order (kz_model_range_site_name's order)
    // (kz_model_range_profile_fast's engine — the one-launch exact-f32 tower — hands range_out to the launch's PROFILE instance
    // instead, which fills all of it: kz_engine_forward.hpp)
    // range_hist (kz_model_range_histogram and _fast): the same engines in histogram mode — range_out holds 64-bit counters
    // [n_sites][KZ_RANGE_BINS] instead, zero at creation, and every pass ADDS the binade counts of what it stores
    void *range_out = nullptr;
    bool range_hist = false;
    int range_site = 0;

    // the tower taps (kz_model_tower_taps, kz_model_error_profile): a tap engine — the planned one-launch tower, never with its
    // heads — hands tap_out to the launch's tap instance, which stores every site's tensor there as its epilogue rounds it
    // (kz_kernels.hpp: TapOut): [n_sites] tensors of tap_boards boards, tap_site_bytes() apart whatever the element.  Filled with
    // 0xff bytes before every pass — a NaN in each of the four elements —, so an element no lane wrote reads as NaN.
    unsigned char *tap_out = nullptr;
    int tap_boards = 0;
    size_t tap_site_bytes() const { return (size_t)tap_boards * model->h * model->w * model->channels * 4; }
    kz::TapOut taps() const { return kz::TapOut{tap_out, tap_site_bytes()}; }
    // the element of a site's tensor: the family's, and at the last site what the plain tower hands on
    kz::TapFormat tap_format(int site) const {
        const bool last = site == 2 * model->depth;
        switch (plan.tower) {
            case Tower::resident_f32: return kz::TapFormat::f32;
            case Tower::resident_split16: return last ? kz::TapFormat::f32 : kz::TapFormat::split16;
            case Tower::resident_bf16g: return last ? kz::TapFormat::f32 : kz::TapFormat::bf16;
            default: return kz::TapFormat::f16;  // resident_f16, resident_f16g
        }
    }
    const unsigned char *tap_site(int site) const { return tap_out + (size_t)site * tap_site_bytes(); }
    // site `site` of this tap engine's last pass (`boards` boards) against the same rows in exact f32 (row stride ref_ld floats)
    int tap_deviation(const Pass &p, int site, const float *ref, int ref_ld, int boards, kz::TapDeviation *out) const {
        kz::launch_tap_deviation(tap_site(site), tap_format(site), tap_site_bytes() / 2, model->channels, ref, ref_ld,
                                 (size_t)boards * model->h * model->w, out_channels, out, p.stream);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // the error profile's per-layer reference (an exact-f32 profiling engine): instead of a maximum, every stash site is compared
    // with tap_peer's tap of that site (tap_peer has finished its pass), into deviation [n_sites] in device memory
    const kz_engine *tap_peer = nullptr;
    kz::TapDeviation *deviation = nullptr;
    kz::Int8SiteDeviation *deviation8 = nullptr;  // instead, where tap_peer is an int8 tap engine (kz_model_int8_error_profile)

    // The int8 taps (kz_model_int8_taps, kz_model_int8_error_profile): a tap engine of resident_i8 or board_conv_i8.  A site's
    // tensor holds the int8 image at its start and the f16 stream value stored beside it tap_site_bytes() / 2 behind (mid sites
    // have no stream, the last site no image).  The image part is filled with 0x80 before a pass (tap_fill): -128 is what no
    // lane wrote.  The one-launch tower's tap instance writes rows of model->channels elements; the per-layer plan's images and
    // stream rows are copied behind each layer's launch and keep the engine's own strides, C8 bytes and cp halves.
    // tap_geometry_batch: the batch whose wide level a tap launch runs (the int8 launch chooses its level per launch).
    int tap_geometry_batch = 0;
    int tap_image_ld() const { return plan.tower == Tower::board_conv_i8 ? wts->c8 : model->channels; }
    int tap_stream_ld() const { return plan.tower == Tower::board_conv_i8 ? cp : model->channels; }
    const unsigned char *tap_stream(int site) const { return tap_site(site) + tap_site_bytes() / 2; }
    int tap_fill(const Pass &p) {
        const size_t n = (size_t)(2 * model->depth + 1), sb = tap_site_bytes();
        if (!i8()) {
            HIP_TRY(hipMemsetAsync(tap_out, 0xff, n * sb, p.stream));
            return 0;
        }
        for (size_t site = 0; site < n; site++) {
            HIP_TRY(hipMemsetAsync(tap_out + site * sb, 0x80, sb / 2, p.stream));
            HIP_TRY(hipMemsetAsync(tap_out + site * sb + sb / 2, 0xff, sb / 2, p.stream));
        }
        return 0;
    }
    // (board_conv_i8, a tap engine) a layer's image and f16 rows to the site's tensors, behind that layer's launch
    int tap_copy(const Pass &p, int site, const void *image, const void *stream16, int batch) {
        const size_t rows = (size_t)batch * model->h * model->w;
        if (image) HIP_TRY(hipMemcpyAsync(tap_out + (size_t)site * tap_site_bytes(), image, rows * wts->c8, hipMemcpyDeviceToDevice, p.stream));
        if (stream16)
            HIP_TRY(hipMemcpyAsync(tap_out + (size_t)site * tap_site_bytes() + tap_site_bytes() / 2, stream16, rows * cp * 2, hipMemcpyDeviceToDevice, p.stream));
        return 0;
    }
    // both reductions of site `site` of this int8 tap engine's last pass against the same rows in exact f32
    int tap_deviation8(const Pass &p, int site, const float *ref, int ref_ld, int boards, kz::Int8SiteDeviation *out) const {
        const size_t rows = (size_t)boards * model->h * model->w;
        const int n = 2 * model->depth + 1;
        if (site < n - 1)
            kz::launch_tap_deviation_i8(tap_site(site), tap_image_ld(), model->i8_exp[site], ref, ref_ld, rows, out_channels, out, p.stream);
        if (site % 2 == 0)
            kz::launch_tap_deviation(tap_stream(site), kz::TapFormat::f16, 0, tap_stream_ld(), ref, ref_ld, rows, out_channels, &out->stream, p.stream);
        HIP_TRY(hipGetLastError());
        return 0;
    }

    int stash(const Pass &p, const std::string &name, const void *src, int batch) {
        if (!plan.keep) return 0;
        if (tap_peer) {
            const int site = range_site++;
            if (deviation8) return tap_peer->tap_deviation8(p, site, (const float *)src, cp, batch, deviation8 + site);
            return tap_peer->tap_deviation(p, site, (const float *)src, cp, batch, deviation + site);
        }
        if (range_hist) {
            unsigned long long *out = (unsigned long long *)range_out + (size_t)range_site++ * kz::RANGE_BINS;
            return launch(p, "kz_range_histogram", [&] {
                kz::launch_range_histogram((const float *)src, batch, model->h * model->w, model->channels, cp, out, p.stream);
            });
        }
        if (range_out) {
            float *out = (float *)range_out + (size_t)range_site++ * max_batch;
            return launch(p, "kz_range_absmax", [&] {
                kz::launch_range_absmax((const float *)src, batch, model->h * model->w, model->channels, cp, out, p.stream);
            });
        }
        const size_t bytes = (size_t)batch * model->h * model->w * cp * esz;
        auto it = kept.find(name);
        if (it == kept.end()) {
            void *buf = nullptr;
            if (dmalloc(&buf, (size_t)max_batch * model->h * model->w * cp * esz)) return 1;
            it = kept.emplace(name, buf).first;
        }
        HIP_TRY(hipMemcpyAsync(it->second, src, bytes, hipMemcpyDeviceToDevice, p.stream));
        return 0;
    }

    // ---- the forward pass (kz_engine_forward.hpp) ----
    // the bracket of every launch: `enqueue` starts kernel `name` (the profiler's and kz_engine_kernel_time's name) on p.stream
    template <class F>
    int launch(const Pass &p, const char *name, F &&enqueue) {
        prof.begin(name, p.stream);
        enqueue();
        prof.end(p.stream);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // the boards of an entry point as the launches take them (kz_kernels.hpp): the model's plane counts go with the pointers
    // sym: the batch's symmetry ids (the engine's tables go with them)
    kz::PackedBoards packed_boards(const void *bits, size_t stride, const void *scalars, const uint8_t *sym = nullptr) const {
        kz::PackedBoards in{(const uint8_t *)bits, stride, (const float *)scalars, model->n_scalar, model->n_bool};
        if (sym) {
            in.n_sym = n_sym;
            in.sym = sym;
            in.square_src = d_square_src;
        }
        return in;
    }
    // the caller's boards into a slot's pinned input staging, rows packed to bits_bytes()
    void stage_boards(Slot &s, const uint8_t *bits, size_t stride, const float *scalars, int batch) const {
        const size_t bb = bits_bytes();
        for (int b = 0; b < batch; b++) memcpy(s.h_bits + b * bb, bits + b * stride, bb);
        if (model->n_scalar) memcpy(s.h_sin, scalars, (size_t)batch * model->n_scalar * 4);
    }
    // ... and, where the launches do not read the pinned staging themselves, on to the slot's device copies
    int copy_boards_in(const Pass &p, Slot &s, int batch) const {
        HIP_TRY(hipMemcpyAsync(s.d_bits, s.h_bits, batch * bits_bytes(), hipMemcpyHostToDevice, p.stream));
        HIP_TRY(hipMemcpyAsync(s.d_sin, s.h_sin, (size_t)batch * model->n_scalar * 4, hipMemcpyHostToDevice, p.stream));
        return 0;
    }
    int conv(const Pass &p, const DevConv &w, const void *x, int ldx, void *y, int ldy, int M, int relu, const void *res, bool post,
             int h, int wd, int group, int src_group, int src_off, float *y32 = nullptr, int ldy32 = 0);
    // packed: boards still to be encoded (the one-launch towers encode inside the launch)
    int run_tower(const Pass &p, int batch, float *d_scalars, float *d_policy, const kz::PackedBoards *packed = nullptr,
                  const kz::DecodeArgs *dec = nullptr);
    bool extra_in_scalar_head() const;
    kz::ScalarHeadArgs scalar_head_args(const ScalarBranch &s, const void *x, int batch, int hc, int hs, float *out) const;
    int run_heads(const Pass &p, int batch, float *d_scalars, float *d_policy);
    int forward_packed(const Pass &p, const kz::PackedBoards &in, int batch, void *d_sout, void *d_pol, const kz::DecodeArgs *dec = nullptr);
    int forward_dense(const Pass &p, const void *d_nchw, int batch, void *d_sout, void *d_pol);
};
