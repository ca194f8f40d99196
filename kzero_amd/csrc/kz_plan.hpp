// kz_plan.hpp — which kernels run a network.  Part of kz_engine.hip's translation unit (included inside its anonymous
// namespace); exported through kz_model_plan and kz_model_supports_dtype.
#pragma once

// ------------------------------------------------------------------------------------------------
// Which kernels run a network: pure host logic over the kernels' support predicates (no HIP call), shared by
// kz_engine_create and kz_model_plan — DESIGN.md §5 prints its table from it and tests/test_path_table.py holds it, and
// the environment switches' effect on it, to tests/golden/path_table.json without a GPU.  plan_path is the first-match
// chain below; its answer, one PathPlan, is the tower's kernel family plus the few choices independent of it.  The engine
// keeps the plan and asks it (the functions below) whatever depends on it; DeviceWeights::build reads its WeightsSpec.
//
//   dtype f16:         8x8, 256 channels, <= 224 planes          -> tower_resident_f16 [+heads: attention head, Q = 256]
//                      else a shape of kz_tower_split.hip        -> tower_resident_f16g [+heads: conv heads at 128 / 256]
//                      else channels % 64 == 0, >= 160 workgroups -> board_conv_f16          (one launch per layer)
//                      else                                       -> conv_igemm_f16          (one launch per layer)
//   dtype f32:         128 / 256 channels on a small board        -> tower_resident_f32 [+heads: conv heads]
//                      else                                       -> conv_igemm_f32
//   dtype f32split16:  a shape of kz_tower_split.hip (split)      -> tower_resident_split16 [+heads]
//                      else channels % 64 == 0                    -> board_conv_split16      (one launch per layer)
//                      else                                       -> refused (kz_model_supports_dtype says 0)
//   dtype bf16 (3):    a shape of kz_tower_f16g.hip               -> tower_resident_bf16g [+heads: conv heads at 128 / 256]
//                      else                                       -> refused
//   dtype int8 (4):    a calibrated model (kz_model_quantize_int8) of a shape of kz_tower_i8.hip -> tower_resident_i8
//                      else                                       -> refused (the message says which of the two is missing)
//   dtype int8 + heads (5): dtype 4's tower; a conv policy head and a scalar head the tail takes on the narrow tiles
//                      (kz::tower_i8_conv_heads_supported) -> tower_resident_i8+heads, one launch; else -> exactly dtype 4's plan
//                      Either takes the wide tiles (more boards per workgroup, chosen per launch from its batch) where
//                      max_batch fills a wide level; with the heads inside no level wider than the tail fits (wide_cap)
//   dtype int8, any shape (8): exactly dtype 5's plan wherever dtype 5 has one; else, on a calibrated model with at least one
//                      block, a board of 2 .. 32 squares a side that fits a workgroup of the board-tile kernels and at most
//                      512 channels once widened to a multiple of 128 -> board_conv_i8 (one launch per layer, the f16
//                      engine's encode and heads around it; NO >= 160-workgroup condition: the alternative is a refusal)
//                      else                                       -> refused
// ------------------------------------------------------------------------------------------------
//   AttentionTower (attention.py) instead of the ResTower:
//     8x8, 8 heads of d_k = d_v = 16, d_model 128 / 256: dtype f16 -> attention_tower_f16, f32 -> attention_tower_f32 (the same
//                                                       launch on v_mfma_f32_16x16x4_f32; d_ff <= 256)
//     any other shape (f32, or f16 rows around f32 arithmetic)   -> attention_tower_f32_valu (one launch, vector ALUs)
//     f32split16, bf16, int8                                     -> refused
//   DenseNetwork (simple.py: no tower, no heads), f32 / f16         -> dense_network_f32 (one launch, f32 arithmetic)

// the kernel family that runs the tower (path_name: the name kz_model_plan / kz_engine_tower_path report)
enum class Tower {
    dense_net,           // kz_dense_network.hip: the whole network, f32 arithmetic
    att_valu,            // kz_att_tower.hip: AttentionTower on the vector ALUs
    att_mfma,            // kz_att_tower_mfma.hip: AttentionTower on the matrix cores, in the engine's arithmetic
    resident_f16,        // kz_tower.hip: the chess network's one launch
    resident_f32,        // kz_tower_f32.hip: exact f32, one launch
    resident_split16,    // kz_tower_split.hip: split arithmetic, one launch
    resident_f16g,       // kz_tower_f16g.hip: the split kernel without its lo halves — plain f16, generic shapes
    resident_bf16g,      // kz_tower_bf16g.hip: that plain kernel on bf16 elements, f32 tensors around it
    resident_i8,         // kz_tower_i8.hip: int8 block convolutions beside an f16 residual stream, f16 tensors around it
    board_conv_f16,      // kz_board_conv.hip: one launch per layer, whole boards as LDS tiles
    board_conv_split16,  // the same per layer in split arithmetic (boards the one-launch split tower cannot hold)
    board_conv_i8,       // kz_board_conv_i8.hip: the same per layer on the i8 matrix cores, int8 images beside the f16 stream
    conv_igemm,          // kz_kernels.hip: one implicit GEMM per layer
};

struct PathPlan {
    Tower tower = Tower::conv_igemm;
    bool heads = false;      // the tower launch runs the heads too ("+heads"), and can end in decode_output
    bool wide = false;       // resident_f16g with more boards per workgroup (kz::tower_split_wide_supported); resident_i8: tower_i8_wide_supported
    int wide_cap = 0;        // resident_i8, wide with the heads inside: the widest wide level whose tail fits, in tiles (0: the tower alone)
    bool att_heads = false;  // heads in launches of their own: ScalarHead + AttentionPolicyHead as one (kz_att_heads.hip)
    bool keep = false;       // KZ_KEEP_ACTIVATIONS: the per-layer path keeps every layer's output
    int tower_nb = 2;        // KZ_TOWER_NB: boards per workgroup of the resident_f16 launch at up to 32 input planes (1 or 2)
    int launches = 0;        // kernel launches per batch through the packed-input entry points
#ifdef KZ_EXPERIMENTS
    // the experiment build's switches (kz_engine.hip: experiment_switches): KZ_TOWER_NB=4, KZ_TOWER_PREV, KZ_T32_BOARDS=3,
    // KZ_BOARD_CONV2, KZ_HIP_GRAPH, KZ_NO_ZERO_COPY
    bool nb4 = false, tower_prev = false, t32_dense3 = false, conv2 = false, graph = false, no_zero_copy = false;
#endif
};

// KZ_DTYPE_F32_SPLIT16: the f32 engine (dtype KZ_DTYPE_F32) with split arithmetic in the tower and the 1x1 head convolutions
bool split_arithmetic(Tower t) { return t == Tower::resident_split16 || t == Tower::board_conv_split16; }
bool split_arithmetic(const PathPlan &p) { return split_arithmetic(p.tower); }

// What the device weights depend on of a plan — all that DeviceWeights::build (kz_device_weights.hpp) is given of it, and with
// the model, the device and the dtype the key of the weights cache: plans of equal spec share one set of streams.
enum class StreamHeads { none, attention, conv };  // the heads whose weights ride in the one-launch tower's stream
struct WeightsSpec {
    Tower tower = Tower::conv_igemm;
    StreamHeads heads = StreamHeads::none;
    bool att_heads = false;              // PathPlan::att_heads: the attention policy head packed for kz_att_heads.hip
    bool conv2 = false, nb4 = false;     // PathPlan::conv2, nb4 (the experiment build; false in the product)
    auto fields() const { return std::tie(tower, heads, att_heads, conv2, nb4); }
    bool operator<(const WeightsSpec &o) const { return fields() < o.fields(); }
};
WeightsSpec weights_spec(const Model &m, const PathPlan &p) {
    WeightsSpec s;
    s.tower = p.tower;
    if (p.heads) s.heads = m.policy_kind == kz::POLICY_ATTENTION ? StreamHeads::attention : StreamHeads::conv;
    // the exact-f32 stream carries the conv heads wherever the kernel can run them, whether the launch does or not: one
    // stream for "+heads", for KZ_NO_FUSED_HEADS and for the range profile's engine
    if (p.tower == Tower::resident_f32)
        s.heads = kz::tower32_heads_supported((int)m.policy_kind, m.policy_extra_moves, m.policy_conv_channels, m.h, m.w, m.channels,
                                              m.sh_conv.cout, m.sh_fc0.out)
                      ? StreamHeads::conv
                      : StreamHeads::none;
    s.att_heads = p.att_heads;
#ifdef KZ_EXPERIMENTS
    s.conv2 = p.conv2;
    s.nb4 = p.nb4;
#endif
    return s;
}

// one launch per layer (stem + 2·depth convolutions) through three rotating activation buffers; else one launch, one buffer
bool per_layer(const PathPlan &p) {
    return p.tower == Tower::board_conv_f16 || p.tower == Tower::board_conv_split16 || p.tower == Tower::board_conv_i8 || p.tower == Tower::conv_igemm;
}

// the tower launch reads the packed boards itself (no encode launch in front of it)
bool encodes_boards(const PathPlan &p) { return !per_layer(p) && p.tower != Tower::dense_net && p.tower != Tower::att_valu; }

// dtype: KZ_DTYPE_F32 / KZ_DTYPE_F16 (/ KZ_DTYPE_F32_SPLIT16, whose towers are all split; / bf16, whose tower is resident_bf16g)
const char *path_name(const PathPlan &p, int dtype) {
    const bool f16 = dtype == KZ_DTYPE_F16;
    switch (p.tower) {
        case Tower::dense_net: return "dense_network_f32";
        case Tower::att_valu: return "attention_tower_f32_valu";
        case Tower::att_mfma: return f16 ? "attention_tower_f16" : "attention_tower_f32";
        case Tower::resident_f16: return p.heads ? "tower_resident_f16+heads" : "tower_resident_f16";
        case Tower::resident_f32: return p.heads ? "tower_resident_f32+heads" : "tower_resident_f32";
        case Tower::resident_split16: return p.heads ? "tower_resident_split16+heads" : "tower_resident_split16";
        case Tower::resident_f16g: return p.heads ? "tower_resident_f16g+heads" : "tower_resident_f16g";
        case Tower::resident_bf16g: return p.heads ? "tower_resident_bf16g+heads" : "tower_resident_bf16g";
        case Tower::resident_i8: return p.heads ? "tower_resident_i8+heads" : "tower_resident_i8";
        case Tower::board_conv_f16: return "board_conv_f16";
        case Tower::board_conv_split16: return "board_conv_split16";
        case Tower::board_conv_i8: return "board_conv_i8";
        case Tower::conv_igemm: return f16 ? "conv_igemm_f16" : "conv_igemm_f32";
    }
    return "";
}

bool env_on(const char *name) {
    const char *v = getenv(name);
    return v && v[0] == '1';
}

// the f16 engines' one-launch ScalarHead + AttentionPolicyHead (kz_att_heads.hip)
bool att_heads_one_launch(const Model &m, int dtype) {
#ifdef KZ_EXPERIMENTS
    if (env_on("KZ_NO_ATT_HEADS")) return false;  // (A/B against the four separate launches)
#endif
    return m.policy_kind == kz::POLICY_ATTENTION && dtype == KZ_DTYPE_F16 &&
           kz::att_heads_supported(dtype, m.h, m.w, m.channels, m.policy_query_channels, m.sh_conv.cout, m.sh_fc0.out, m.policy_len);
}

// launches of run_heads for a network whose tower output is materialised (head convolutions with cout_p = round_up(cout, 32))
int head_launches(const Model &m, int dtype, const PathPlan &p, int cp) {
    if (p.att_heads) return 1;
    int n = 1;  // kz_scalar_head
    const bool f16_heads = split_arithmetic(p) || dtype == KZ_DTYPE_F16;  // 1x1 head convolutions through kz_conv1x1_split where it fits
    switch (m.policy_kind) {
        case kz::POLICY_ATAXX_CONV:
        case kz::POLICY_CONV: {
            const int c0_in = round_up(m.p_conv0.cin, 32), c0_out = round_up(m.p_conv0.cout, 32);
            const bool one = m.policy_kind == kz::POLICY_CONV && f16_heads && kz::conv1x1_split_supported(c0_in, c0_out) && cp >= c0_in &&
                             kz::conv1x1_policy_epilogue_supported(c0_in, c0_out, m.p_conv0.cout, m.policy_conv_channels);
            n += one ? 1 : 2;
            if (m.policy_kind == kz::POLICY_CONV && m.policy_extra_moves) {
                const bool in_scalar_head = m.sh_conv.cout == 4 && m.p_extra_conv.cout == 1 && m.p_extra_conv.cin == m.sh_conv.cin &&
                                            kz::scalar_head_takes_extra(dtype == KZ_DTYPE_F32 ? 0 : 1, cp, m.sh_conv.cout);
                n += in_scalar_head ? 0 : 1;
            }
            break;
        }
        case kz::POLICY_ATTENTION: n += 3; break;
        case kz::POLICY_ARIMAA: n += 3; break;  // bulk: two 1x1 convolutions; the scalar branch through kz_scalar_head
        case kz::POLICY_DENSE: n += (m.dense_hidden_channels ? 1 : 0) + (m.dense_hidden_size ? 2 : 1); break;
        case kz::POLICY_NONE: return 0;
    }
    return n;
}

// the int8 dtypes: one one-launch tower; 5 with the conv heads inside its launch where the launch can carry them; 8 is 5 with
// the per-layer int8 kernel behind it for the shapes that tower refuses
bool int8_dtype(int dtype) { return dtype == KZ_DTYPE_INT8 || dtype == KZ_DTYPE_INT8_HEADS || dtype == KZ_DTYPE_INT8_ANY; }

// dtype_in: KZ_DTYPE_F32 / KZ_DTYPE_F16 / KZ_DTYPE_F32_SPLIT16 / KZ_DTYPE_BF16 / int8 (4, 5).  false + why: kz_engine_create refuses.
// (The messages say "bf16" or "dtype 3", "int8" or "dtype 4" / "dtype 5" / "dtype 8": the library's strings name no KZ_ identifier but the documented ones.)
bool plan_path(const Model &m, int max_batch, int dtype_in, PathPlan &p, std::string &why) {
    const bool split16 = dtype_in == KZ_DTYPE_F32_SPLIT16, bf16 = dtype_in == KZ_DTYPE_BF16, i8 = int8_dtype(dtype_in);
    const std::string i8_name = "(dtype " + std::to_string(dtype_in) + ")";  // in the int8 messages: the value the caller gave
    // split16 and bf16 are the f32 engine with the tower's launch exchanged, int8 is the f16 engine with it exchanged
    const int dtype = split16 || bf16 ? KZ_DTYPE_F32 : i8 ? KZ_DTYPE_F16 : dtype_in;
    const int cp = round_up(m.channels, 32);
    const bool force = env_on("KZ_FORCE_GENERIC"), nofuse = env_on("KZ_NO_FUSED_HEADS");
    p = PathPlan();
    // dtype 4 (and 5) exists for a calibrated model only: to a model as loaded it is what it was before there was an int8
    // arithmetic, an unknown dtype — said first, then which of the two, calibration or kernel, is missing
    const std::string i8_pre = i8 && m.i8_exp.empty() ? "unknown dtype " + std::to_string(dtype_in) + " for a model that carries no int8 calibration (kz_model_quantize_int8 makes one that does): " : "";
    if (m.tower_kind == kz::TOWER_DENSE_NET) {  // DenseNetwork (simple.py): the whole network is one launch behind the encode
        if (i8) {
            why = i8_pre + "the int8 arithmetic " + i8_name + " has no DenseNetwork kernel: a network without a tower runs in f32 arithmetic (dtype f32, or f16 rows around it)";
            return false;
        }
        if (bf16) {
            why = "the bf16 arithmetic (dtype 3) has no DenseNetwork kernel: a network without a tower runs in f32 arithmetic (dtype f32, or f16 rows around it)";
            return false;
        }
        if (split16) {
            why = "KZ_DTYPE_F32_SPLIT16 has no DenseNetwork kernel: such a network runs in f32 arithmetic (KZ_DTYPE_F32, or KZ_DTYPE_F16 rows around it)";
            return false;
        }
        if (!kz::dense_network_supported(m.h, m.w, m.c_in, m.channels, m.depth, m.policy_len)) {
            why = "dense network: the board's input vector and the hidden vectors do not fit the LDS of one workgroup";
            return false;
        }
        p.tower = Tower::dense_net;
        p.launches = 2;
        return true;
    }
    if (m.tower_kind == kz::TOWER_ATTENTION) {
        if (i8) {
            why = i8_pre + "the int8 arithmetic " + i8_name + " has no attention-tower kernel: an AttentionTower network runs in exact f32 or in f16";
            return false;
        }
        if (bf16) {
            why = "the bf16 arithmetic (dtype 3) has no attention-tower kernel: an AttentionTower network runs in exact f32 or in f16";
            return false;
        }
        if (split16) {
            why = "KZ_DTYPE_F32_SPLIT16 has no attention-tower kernel: an AttentionTower network runs as KZ_DTYPE_F32 (exact) or KZ_DTYPE_F16";
            return false;
        }
        if (!kz::att_tower_supported(m.h, m.w, m.c_in, m.channels, m.att_heads, m.att_dk, m.att_dv, m.att_dff, m.depth)) {
            why = "attention tower: the token matrix of one board (squares x d_model) with one head's q, k, v and all heads' "
                  "outputs beside it does not fit the 160 KB of LDS of one workgroup, or the board has more than 384 squares";
            return false;
        }
        // the matrix-core launch, in the engine's arithmetic — f16, or exact f32
        p.tower = !force && kz::att_tower16_supported(m.h, m.w, m.c_in, m.channels, m.att_heads, m.att_dk, m.att_dv, m.att_dff, m.depth,
                                                      dtype == KZ_DTYPE_F32)
                      ? Tower::att_mfma
                      : Tower::att_valu;
    } else if (i8) {
        // the one-launch int8 tower or nothing; of the switches it reads none (it has one tower), and the heads behind it are
        // the f16 engine's — or, dtype 5, inside the launch where its tail takes them
        if (m.depth < 1) {
            why = i8_pre + "the int8 arithmetic " + i8_name + " needs a tower with at least one residual block: only the block convolutions are quantised";
            return false;
        }
        const bool one_launch = kz::tower_i8_supported(m.h, m.w, m.channels, m.depth, m.c_in);
        if (!one_launch && dtype_in == KZ_DTYPE_INT8_ANY && !m.i8_exp.empty()) {
            // dtype 8 behind the one-launch tower: the per-layer int8 kernel, or a refusal (no other kernel, no workgroup floor).
            // (A model that carries no calibration is told what dtype 4 tells it, below.)
            if (!kz::board_conv_i8_supported(m.h, m.w, m.channels) || m.tower.empty() || m.tower[0].k != 3) {
                why = i8_pre + "the int8 arithmetic " + i8_name + " has no kernel for this shape (the model is calibrated): neither the one-launch int8 tower nor the per-layer int8 kernel (board_conv_i8) takes it — per layer a board "
                      "has 2 to 32 squares a side and fits the 24 tiles of 16 squares and the LDS of a workgroup, and the tower has at "
                      "most 512 channels once widened to a multiple of 128";
                return false;
            }
            if (m.i8_exp.size() != (size_t)(2 * m.depth)) {
                why = i8_pre + "the int8 arithmetic " + i8_name + " needs a calibrated model (the shape has a kernel, the calibration is missing): make one with "
                      "kz_model_quantize_int8 from the site maxima of kz_model_range_profile_fast";
                return false;
            }
            p.tower = Tower::board_conv_i8;
            p.att_heads = att_heads_one_launch(m, dtype);
            p.launches = 2 + 2 * m.depth + head_launches(m, dtype, p, cp);  // encode, the stem, the block convolutions, the f16 heads
            return true;
        }
        if (!one_launch) {
            why = i8_pre + "the int8 arithmetic " + i8_name + " has no kernel for this shape (" + std::string(m.i8_exp.empty() ? "and the model is not calibrated either" : "the model is calibrated") +
                  "): the one-launch int8 tower takes 256 tower channels (193 to 255 run widened to 256) on a board of at most 64 "
                  "squares with at most 128 input planes, and 128 (65 to 127 widened) on at most 96 squares with at most 64 input "
                  "planes; 64 channels or fewer, 129 to 192 and more than 256 have no int8 kernel";
            return false;
        }
        if (m.i8_exp.size() != (size_t)(2 * m.depth)) {
            why = i8_pre + "the int8 arithmetic " + i8_name + " needs a calibrated model (the shape has a kernel, the calibration is missing): make one with "
                  "kz_model_quantize_int8 from the site maxima of kz_model_range_profile_fast";
            return false;
        }
        p.tower = Tower::resident_i8;
        p.wide = kz::tower_i8_wide_supported(m.h, m.w, m.channels, max_batch);
        // one launch per batch — zero-copy slots, the decode inside — is worth more than wider tiles (the precedent of
        // resident_f16g below): the narrow tiles decide `heads`, and the plan is then wide only up to the level whose tail fits
        if (dtype_in != KZ_DTYPE_INT8 && kz::tower_i8_conv_heads_supported((int)m.policy_kind, m.policy_extra_moves, m.policy_conv_channels,
                                                                                 m.h, m.w, m.channels, m.sh_conv.cout, m.sh_fc0.out)) {
            p.heads = true;
            p.wide_cap = kz::tower_i8_conv_heads_wide_cap((int)m.policy_kind, m.policy_extra_moves, m.policy_conv_channels, m.h, m.w, m.channels,
                                                          m.sh_conv.cout, m.sh_fc0.out);
            p.wide = p.wide_cap != 0 && kz::tower_i8_wide_supported(m.h, m.w, m.channels, max_batch, p.wide_cap);
            if (!p.wide) p.wide_cap = 0;
        }
    } else if (!force && kz::tower_resident_supported(dtype, m.h, m.w, m.channels, m.depth, m.c_in)) {  // (f16 only)
        p.tower = Tower::resident_f16;
        if (const char *nb = getenv("KZ_TOWER_NB"); nb && atoi(nb) == 1) p.tower_nb = 1;
        p.heads = !nofuse && kz::tower_heads_supported((int)m.policy_kind, m.policy_query_channels, m.policy_len, m.sh_conv.cout,
                                                       m.sh_fc0.out);
    } else {
        // the per-layer activation taps of KZ_KEEP_ACTIVATIONS need a per-layer path (the one-launch split tower ignores
        // them, and KZ_FORCE_GENERIC too: DESIGN.md §5)
        p.keep = env_on("KZ_KEEP_ACTIVATIONS");
        if (bf16) {
            // the one-launch tower of the plain-f16 family or nothing (like the one-launch split tower it ignores
            // KZ_FORCE_GENERIC and KZ_KEEP_ACTIVATIONS); the heads, where not inside, are the f32 engine's
            p.keep = false;
            if (m.depth < 1) {
                why = "the bf16 arithmetic (dtype 3) needs a tower with at least one residual block: without blocks there is no "
                      "residual stream to keep in range, and the stem alone runs as exact f32";
                return false;
            }
            if (!kz::tower_split_supported(m.h, m.w, m.channels, m.depth, m.c_in, false)) {
                why = "the bf16 arithmetic (dtype 3) has the one-launch tower only: 64 to 512 tower channels in a multiple of 64 on a "
                      "board that fits a workgroup's LDS (256 / 320 channels on at most 96 squares, 384 / 512 on at most 64, 192 on "
                      "at most 176, 128 on at most 208, 64 on at most 96) with no more input planes than tower channels; a "
                      "larger board (Go 19x19) runs per layer, which has no bf16 kernel";
                return false;
            }
            p.tower = Tower::resident_bf16g;
            const auto conv_heads = [&](int wide_batch) {
                return !nofuse && kz::tower_split_conv_heads_supported((int)m.policy_kind, m.policy_extra_moves, m.policy_conv_channels, m.h,
                                                                       m.w, m.channels, m.sh_conv.cout, m.sh_fc0.out, false, wide_batch);
            };
            p.wide = kz::tower_split_wide_supported(m.h, m.w, m.channels, max_batch);
            p.heads = conv_heads(p.wide ? max_batch : 0);
            if (p.wide && !p.heads && conv_heads(0)) {  // (as for resident_f16g below: one launch per batch before wide tiles)
                p.wide = false;
                p.heads = true;
            }
        } else if (split16) {
            if (kz::tower_split_supported(m.h, m.w, m.channels, m.depth, m.c_in, true)) {
                p.tower = Tower::resident_split16;  // same tensors in and out as the exact-f32 resident launch
                p.heads = !nofuse && (kz::tower_split_heads_supported((int)m.policy_kind, m.policy_query_channels, m.policy_len, m.h, m.w,
                                                                      m.channels, m.sh_conv.cout, m.sh_fc0.out) ||
                                      kz::tower_split_conv_heads_supported((int)m.policy_kind, m.policy_extra_moves, m.policy_conv_channels,
                                                                           m.h, m.w, m.channels, m.sh_conv.cout, m.sh_fc0.out, true));
            } else if (m.depth >= 1 && !p.keep && kz::board_conv_split_supported(m.h, m.w, m.channels, m.channels) && m.channels % 32 == 0 &&
                       (size_t)max_batch * m.h * m.w * m.channels * 4 < ((size_t)1 << 31)) {
                p.tower = Tower::board_conv_split16;  // split arithmetic per layer for boards the resident launch cannot hold (Go 19x19)
            } else {
                why = "KZ_DTYPE_F32_SPLIT16 needs a shape of the one-launch split tower (256 tower channels on a board of at most 64 "
                      "squares, 192 on at most 64, 64 / 128 channels on at most 96 squares, and no more input planes than tower "
                      "channels); or, per layer, tower channels a multiple of 64, at least one block and max_batch * squares * "
                      "channels * 4 bytes < 2 GiB";
                return false;
            }
        } else if (!force && !p.keep && kz::tower32_supported(dtype, m.h, m.w, m.channels, m.depth)) {  // (exact f32 only)
            p.tower = Tower::resident_f32;
            p.heads = !nofuse && kz::tower32_heads_supported((int)m.policy_kind, m.policy_extra_moves, m.policy_conv_channels, m.h, m.w,
                                                             m.channels, m.sh_conv.cout, m.sh_fc0.out);
        } else if (dtype == KZ_DTYPE_F16 && !force && !p.keep && !env_on("KZ_NO_RESIDENT_F16G") &&
                   kz::tower_split_supported(m.h, m.w, m.channels, m.depth, m.c_in, false)) {
            // plain-f16 board-resident tower for the shapes the chess launch (kz_tower.hip) does not take
            p.tower = Tower::resident_f16g;
            const auto conv_heads = [&](int wide_batch) {
                return !nofuse && kz::tower_split_conv_heads_supported((int)m.policy_kind, m.policy_extra_moves, m.policy_conv_channels, m.h,
                                                                       m.w, m.channels, m.sh_conv.cout, m.sh_fc0.out, false, wide_batch);
            };
            p.wide = kz::tower_split_wide_supported(m.h, m.w, m.channels, max_batch);
            p.heads = conv_heads(p.wide ? max_batch : 0);
            // the wide tiles hold more boards per workgroup than the fused conv heads' tail takes (four): where the heads fit
            // the narrow tiles only (128 channels on 5x5: eight boards against four), one launch per batch — zero-copy slots,
            // the decode inside — is worth more than the wide tiles' smaller weight traffic
            if (p.wide && !p.heads && conv_heads(0)) {
                p.wide = false;
                p.heads = true;
            }
        } else if (!env_on("KZ_NO_BOARD_CONV") && m.depth >= 1 && kz::board_conv_supported(dtype, m.h, m.w, m.channels, m.channels) &&
                   kz::board_conv_workgroups(max_batch, m.h, m.w, m.channels) >= 160 &&  // (two workgroups per CU when it is busy)
                   (size_t)max_batch * m.h * m.w * m.channels * 2 < ((size_t)1 << 31)) {  // (32-bit buffer offsets; f16 only)
            p.tower = Tower::board_conv_f16;
        } else {
            p.tower = Tower::conv_igemm;
        }
    }
    p.att_heads = !p.heads && att_heads_one_launch(m, dtype);
    // (encode,) the tower — split per layer: + the stem output's split into (hi, lo) rows —, the heads
    const int tower = per_layer(p) ? 2 + 2 * m.depth + (split_arithmetic(p) ? 1 : 0) : encodes_boards(p) ? 1 : 2;
    p.launches = p.heads ? 1 : tower + head_launches(m, dtype, p, cp);
    return true;
}
