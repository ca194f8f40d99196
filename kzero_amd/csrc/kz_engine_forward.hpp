// kz_engine_forward.hpp — the forward pass of an engine: which kernels run for its plan (kz_engine::plan, kz_plan.hpp: the
// tower family, heads inside its launch or not), in which order, on the stream of the Pass it is given.  Out-of-class definitions of the members kz_engine_state.hpp declares;
// included ONCE, by kz_engine.hip.
#pragma once

inline int kz_engine::conv(const Pass &p, const DevConv &w, const void *x, int ldx, void *y, int ldy, int M, int relu, const void *res, bool post,
         int h, int wd, int group, int src_group, int src_off, float *y32, int ldy32) {
    if (w.bws) {  // whole boards as LDS-resident spatial tiles, split arithmetic: (hi, lo) rows of 2 C halves
        kz::BoardConvArgs b{};
        b.x = x; b.ldx = 2 * ldx; b.weights = w.bws; b.bias = w.b; b.res = res; b.y = y; b.ldy = 2 * ldy;
        b.y32 = y32; b.ldy32 = ldy32;
        b.post_scale = post ? wts->post_scale : nullptr;
        b.post_shift = post ? wts->post_shift : nullptr;
        b.boards = M / (h * wd); b.h = h; b.w = wd; b.cin = w.cin_p; b.cout = w.cout; b.relu = relu;
        return launch(p, "kz_board_conv_split16", [&] { kz::launch_board_conv_split(b, p.stream); });
    }
    if (w.bw) {  // whole boards as LDS-resident spatial tiles
        kz::BoardConvArgs b{};
        b.x = x; b.ldx = ldx; b.weights = w.bw; b.bias = w.b; b.res = res; b.y = y; b.ldy = ldy;
        b.post_scale = post ? wts->post_scale : nullptr;
        b.post_shift = post ? wts->post_shift : nullptr;
        b.boards = M / (h * wd); b.h = h; b.w = wd; b.cin = w.cin_p; b.cout = w.cout; b.relu = relu;
        b.rowmap = wts->bc_rowmap; b.halo = wts->bc_halo; b.n_halo = wts->bc_n_halo;
        return launch(p, "kz_board_conv_f16", [&] {
#ifdef KZ_EXPERIMENTS
            if (w.bw2) kz::launch_board_conv2(b, p.stream);
            else
#endif
            kz::launch_board_conv(b, p.stream);
        });
    }
    if (w.sw && y && !res && !post && !y32 && ldx >= w.cin_p) {  // 1x1 head convolution: split16 or any f16 path
        kz::Conv1x1SplitArgs c{};
        c.split = split16();
        c.x = x; c.ldx = ldx; c.weights = w.sw; c.bias = w.b; c.y = y; c.ldy = ldy;
        c.M = M; c.cin_p = w.cin_p; c.cout_p = w.cout_p; c.relu = relu;
        c.group = group; c.src_group = src_group; c.src_off = src_off;
        return launch(p, "kz_conv1x1_split", [&] { kz::launch_conv1x1_split(c, p.stream); });
    }
    kz::ConvArgs a{};
    a.x = x; a.ldx = ldx; a.w = w.w; a.bias = w.b; a.res = res; a.ldres = ldy;
    a.post_scale = post ? wts->post_scale : nullptr;
    a.post_shift = post ? wts->post_shift : nullptr;
    a.y = y; a.y32 = y32; a.ldy = ldy; a.ldy32 = ldy32;
    a.M = M; a.h = h; a.w_ = wd; a.group = group; a.src_group = src_group; a.src_off = src_off;
    a.cin_p = w.cin_p; a.cout_p = w.cout_p; a.cout = w.cout; a.k = w.k; a.relu = relu;
    return launch(p, kz::conv_kernel_name(dtype), [&] { kz::launch_conv(dtype, a, p.stream); });
}

// packed != nullptr (encodes_boards(plan) only): the launch encodes the boards itself.  The "+heads" launches (plan.heads) can
// end in decode_output (kz_decode_dev.hpp): with `dec` nothing but the decoded values and the available moves' probabilities
// leave the launch
inline int kz_engine::run_tower(const Pass &p, int batch, float *d_scalars, float *d_policy, const kz::PackedBoards *packed,
              const kz::DecodeArgs *dec) {
    const Model &m = *model;
    const int hw = m.h * m.w, M = batch * hw;
    if (plan.tower == Tower::dense_net) {  // DenseNetwork: encoded planes in x_in -> scalars and policy, one launch
        kz::DenseNetArgs t{};
        t.x0 = x_in; t.in_f16 = dtype == KZ_DTYPE_F16; t.batch = batch; t.hw = hw; t.cin_p = cin_p; t.size = m.channels;
        t.depth = m.depth; t.res = m.dn_res ? 1 : 0; t.policy_len = m.policy_len;
        t.w_in = wts->dn.w_in; t.b_in = wts->dn.b_in; t.blocks = wts->dn.blocks; t.sf = wts->dn.sf; t.tf = wts->dn.tf;
        t.w_out = wts->dn.w_out; t.b_out = wts->dn.b_out; t.scalars = d_scalars; t.policy = d_policy;
        t.nonfinite_flag = p.nf_flag; t.epoch = p.nf_epoch;
        if (launch(p, "kz_dense_network", [&] { kz::launch_dense_network(t, p.stream); })) return 1;
        tower_out = 0;
        return 0;
    }
    if (plan.tower == Tower::att_mfma) {  // AttentionTower on the matrix cores, in the engine's arithmetic
        kz::AttTower16Args t{};
        t.f32 = dtype == KZ_DTYPE_F32;
        t.x0 = x_in; t.cin_p = cin_p; t.w_expand = wts->att.expand16; t.embedding = wts->att.embedding;
        t.w_layers = wts->att.layers16; t.y = act[0]; t.batch = batch; t.depth = m.depth; t.d_model = m.channels;
        t.d_ff = m.att_dff; t.alpha = m.att_alpha; t.eps = m.ln_eps;
        if (packed) t.in = *packed;  // fused board encode
        if (launch(p, t.f32 ? "kz_att_tower_f32" : "kz_att_tower_f16", [&] { kz::launch_att_tower16(t, p.stream); })) return 1;
        tower_out = 0;
        return 0;
    }
    if (plan.tower == Tower::att_valu) {  // AttentionTower: encoded planes in x_in -> tower output rows in act[0], one launch
        kz::AttTowerArgs t{};
        t.x0 = x_in; t.ldx0 = cin_p; t.in_f16 = dtype == KZ_DTYPE_F16; t.c_in = m.c_in;
        t.expand = wts->att.expand; t.embedding = wts->att.embedding; t.layers = wts->att.layers;
        t.y = act[0]; t.ldy = cp; t.out_f16 = dtype == KZ_DTYPE_F16;
        t.batch = batch; t.h = m.h; t.w = m.w; t.depth = m.depth; t.d_model = m.channels; t.heads = m.att_heads;
        t.d_k = m.att_dk; t.d_v = m.att_dv; t.d_ff = m.att_dff; t.alpha = m.att_alpha; t.eps = m.ln_eps;
        if (launch(p, "kz_att_tower_f32_valu", [&] { kz::launch_att_tower(t, p.stream); })) return 1;
        tower_out = 0;
        return 0;
    }
    if (plan.tower == Tower::resident_f16) {
        kz::TowerArgs t{};
        if (packed) t.in = *packed;  // fused board encode
        t.x0 = x_in; t.cin_p = cin_p; t.w_stem = wts->res.w_stem; t.w_tower = wts->res.w_tower;
        t.bias = wts->res.bias; t.post_scale = wts->post_scale; t.post_shift = wts->post_shift;
        t.y = act[0]; t.batch = batch; t.h = m.h; t.w = m.w; t.depth = m.depth;
        t.boards_per_wg = plan.tower_nb;
        t.fused_heads = plan.heads;
        t.sh_w0 = wts->sh.w0; t.sh_b0 = wts->sh.b0; t.sh_w1 = wts->sh.w1; t.sh_b1 = wts->sh.b1;
        t.sh_w2 = wts->sh.w2; t.sh_b2 = wts->sh.b2; t.att_idx = wts->res.att_idx;
        t.scalars = d_scalars; t.policy = d_policy;
        t.nonfinite_flag = p.nf_flag; t.epoch = p.nf_epoch;
        if (dec && plan.heads) t.decode = *dec;
        if (tap_out) {  // a tap engine (no heads in its plan): the tap instance of the same geometry, every site's tensor to tap_out
            t.taps = taps();
            range_site = 2 * m.depth + 1;
        }
#ifdef KZ_EXPERIMENTS
        t.prev = plan.tower_prev;
#endif
        if (launch(p, "kz_tower_resident_f16", [&] {
#ifdef KZ_EXPERIMENTS
                if (plan.nb4) kz::launch_tower_resident4(t, xres, p.stream);
                else
#endif
                kz::launch_tower_resident(t, p.stream);
            }))
            return 1;
        tower_out = 0;
        return 0;
    }
    if (!per_layer(plan)) {  // resident_f32, resident_split16, resident_f16g, resident_bf16g, resident_i8
        kz::Tower32Args t{};
        t.x0 = (const float *)x_in; t.ldx0 = cin_p; t.c_in = m.c_in; t.weights = wts->res.w32; t.bias = wts->res.bias;
        t.post_scale = wts->post_scale; t.post_shift = wts->post_shift;
        t.y = (float *)act[0]; t.ldy = cp; t.batch = batch; t.h = m.h; t.w = m.w; t.channels = m.channels;
        t.depth = m.depth;
        if (packed) t.in = *packed;  // fused board encode
        if (plan.heads) {  // the scalar head's matrices for either kind of heads, then the kind's own
            kz::Tower32Args::Heads &hd = t.heads;
            const ScalarBranch &sh = wts->sh;
            hd.sh_b0 = sh.b0; hd.sh_b1 = sh.b1; hd.sh_w2 = sh.w2; hd.sh_b2 = sh.b2;
            hd.policy_len = m.policy_len;
            hd.scalars = d_scalars; hd.policy = d_policy;
            hd.nonfinite_flag = p.nf_flag; hd.epoch = p.nf_epoch;
            if (m.policy_kind == kz::POLICY_ATTENTION) {  // (the split launch only)
                hd.kind = kz::Tower32Args::Heads::Kind::attention;
                hd.sh_w0 = sh.w0; hd.sh_w1 = sh.w1; hd.att_idx = wts->res.att_idx;
            } else {  // conv policy heads: the f32 tail
                hd.kind = kz::Tower32Args::Heads::Kind::conv;
                hd.hc = m.sh_conv.cout; hd.hs = m.sh_fc0.out;
                hd.small_w = wts->res.small; hd.sh_w1t = sh.w1t;
                hd.pc = m.policy_conv_channels; hd.p_b1 = wts->pol.b1;
                hd.zero_tail = m.policy_kind == kz::POLICY_ATAXX_CONV ? 1 : 0;
                if (m.policy_kind == kz::POLICY_CONV && m.policy_extra_moves) {
                    hd.extra = m.policy_extra_moves;
                    hd.pe_bc = wts->pol.pe_bc; hd.pe_wl = wts->pol.pe_wl; hd.pe_bl = wts->pol.pe_bl;
                }
            }
        }
        if (dec && plan.heads) t.heads.decode = *dec;
#ifdef KZ_EXPERIMENTS
        t.dense3 = plan.t32_dense3;
#endif
        t.wide = plan.wide;
        t.wide_cap = plan.wide_cap;
        if (range_out) {  // the range profile's engine (resident_f32, no heads): the maxima instead of the tower output
            t.profile = true;
            if (range_hist) t.hist = (unsigned long long *)range_out;  // (the counts instead of the maxima)
            else { t.y = (float *)range_out; t.ldy = max_batch; }
            range_site = 2 * m.depth + 1;  // every epilogue of the launch is a site
        }
        if (tap_out) {  // a tap engine (no heads in its plan): the tap instance of the geometry max_batch plans
            t.taps = taps();
            t.tap_wide_batch = i8() ? tap_geometry_batch : max_batch;  // (the int8 launch chooses its level per launch, from its batch)
            range_site = 2 * m.depth + 1;
        }
        const bool f16g = plan.tower == Tower::resident_f16g;
        const char *name = split16() ? "kz_tower_resident_split" : f16g ? "kz_tower_resident_f16g" : bf16() ? "kz_tower_resident_bf16g" : i8() ? "kz_tower_resident_i8" : "kz_tower_resident_f32";
        bool launched = false;  // (the family has a fixed table of instances: a shape outside it launches nothing)
        int nt = 0;
        if (launch(p, name, [&] {
                if (split16()) launched = kz::launch_tower_split(t, p.stream, &nt);
                else if (bf16()) launched = kz::launch_tower_bf16(t, p.stream, &nt);  // f32 tensors, like the split launch
                else if (f16g) launched = kz::launch_tower_pairs(t, p.stream, &nt);  // f16 tensors behind the same pointers
                else if (i8()) launched = kz::launch_tower_i8(t, wts->res.mult, wts->res.qscale, p.stream, &nt);  // f16 tensors too
                else launched = kz::launch_tower32(t, p.stream, &nt);
            }))
            return 1;
        if (!launched)
            return fail(std::string(name) + ": no instance for " + std::to_string(m.channels) + " channels and nt = " + std::to_string(nt) +
                        " tiles of 16 rows" + (plan.heads ? " with the heads inside the launch" : ""));
        tower_out = 0;
        return 0;
    }
    if (plan.tower == Tower::board_conv_split16) {
        // the stem in exact f32 (its inputs are f32 planes), its output split into (hi, lo) halves — an f32 tensor and a
        // (hi, lo) tensor of the same shape have the same size, so the three activation buffers serve both —, the
        // 2·depth tower convolutions in split arithmetic, the last one writing f32 for the heads
        if (wts->stem_split) {  // encoded f32 planes [M][32] -> (hi, lo) rows -> the board-tile kernel, one chunk
            if (launch(p, "kz_split_rows", [&] { kz::launch_split_rows((const float *)x_in, act[2], (size_t)M, cin_p, p.stream); })) return 1;
            if (conv(p, wts->tower[0], act[2], cin_p, act[0], cp, M, 0, nullptr, false, m.h, m.w, hw, hw, 0)) return 1;
        } else {
            if (conv(p, wts->tower[0], x_in, cin_p, act[2], cp, M, 0, nullptr, false, m.h, m.w, hw, hw, 0)) return 1;
            if (launch(p, "kz_split_rows", [&] { kz::launch_split_rows((const float *)act[2], act[0], (size_t)M, cp, p.stream); })) return 1;
        }
        int cur = 0;
        for (int i = 1; i <= m.depth; i++) {
            const int mid = (cur + 1) % 3, nxt = (cur + 2) % 3;
            const bool last = i == m.depth;
            if (conv(p, wts->tower[2 * i - 1], act[cur], cp, act[mid], cp, M, 1, nullptr, false, m.h, m.w, hw, hw, 0)) return 1;
            if (conv(p, wts->tower[2 * i], act[mid], cp, last ? nullptr : act[nxt], cp, M, 1, act[cur], last, m.h, m.w, hw, hw, 0,
                     last ? (float *)act[nxt] : nullptr, cp))
                return 1;
            cur = nxt;
        }
        tower_out = cur;
        return 0;
    }
    if (plan.tower == Tower::board_conv_i8) {
        // the f16 stem storing the stream and X8, then per block conv A: X8 -> Y8 and conv B: Y8 (+ the f16 stream) -> the
        // stream and X8; the last conv B writes the f16 tower output alone, behind the final BN
        const int C8 = wts->c8;
        const auto i8conv = [&](int l, const void *x, const void *res, void *y16, void *y8, bool post) {
            const DeviceWeights::I8Conv &w = wts->i8conv[l];
            kz::BoardConvI8Args b{};
            b.stem = l == 0;
            b.x = x; b.weights = w.w; b.bias = w.bias; b.mult = w.mult; b.res = res; b.y16 = y16; b.y8 = y8; b.qscale = w.qscale;
            b.post_scale = post ? wts->post8_scale : nullptr;
            b.post_shift = post ? wts->post8_shift : nullptr;
            b.ld16 = cp; b.boards = batch; b.h = m.h; b.w = m.w; b.cin = l == 0 ? cin_p : C8; b.cout = C8; b.relu = l != 0;
            return launch(p, l == 0 ? "kz_board_conv_i8_stem" : "kz_board_conv_i8", [&] { kz::launch_board_conv_i8(b, p.stream); });
        };
        // (a tap engine: every layer's image and stream rows to the site's tap tensors behind its launch, on the same stream)
        const bool tap = tap_out != nullptr;
        if (i8conv(0, x_in, nullptr, act[0], act8[0], false)) return 1;
        if (tap && tap_copy(p, 0, act8[0], act[0], batch)) return 1;
        int cur = 0;
        for (int i = 1; i <= m.depth; i++) {
            const int nxt = (cur + 1) % 3;
            const bool last = i == m.depth;
            if (i8conv(2 * i - 1, act8[0], nullptr, nullptr, act8[1], false)) return 1;
            if (tap && tap_copy(p, 2 * i - 1, act8[1], nullptr, batch)) return 1;
            if (i8conv(2 * i, act8[1], act[cur], act[nxt], last ? nullptr : act8[0], last)) return 1;
            if (tap && tap_copy(p, 2 * i, last ? nullptr : act8[0], act[nxt], batch)) return 1;
            cur = nxt;
        }
        if (tap) range_site = 2 * m.depth + 1;
        tower_out = cur;
        return 0;
    }
    // stem: conv + bias, no activation (post_act.py:205)
    range_site = 0;
    if (conv(p, wts->tower[0], x_in, cin_p, act[0], cp, M, 0, nullptr, m.depth == 0, m.h, m.w, hw, hw, 0)) return 1;
    if (stash(p, m.depth == 0 ? "tower.1" : "tower.0", act[0], batch)) return 1;
    int cur = 0;
    for (int i = 1; i <= m.depth; i++) {
        const int mid = (cur + 1) % 3, nxt = (cur + 2) % 3;
        const bool last = i == m.depth;
        if (conv(p, wts->tower[2 * i - 1], act[cur], cp, act[mid], cp, M, 1, nullptr, false, m.h, m.w, hw, hw, 0))
            return 1;
        if (stash(p, "tower." + std::to_string(i) + ".mid", act[mid], batch)) return 1;
        // x + relu(bn(conv(mid))) (post_act.py:227-228); the tower's final BN rides on the last block
        if (conv(p, wts->tower[2 * i], act[mid], cp, act[nxt], cp, M, 1, act[cur], last, m.h, m.w, hw, hw, 0))
            return 1;
        if (stash(p, "tower." + std::to_string(last ? i + 1 : i), act[nxt], batch)) return 1;
        cur = nxt;
    }
    tower_out = cur;
    return 0;
}

inline bool kz_engine::extra_in_scalar_head() const {
    const Model &m = *model;
    return m.policy_kind == kz::POLICY_CONV && m.policy_extra_moves > 0 && wts->pol.w0x &&
           kz::scalar_head_takes_extra(dtype == KZ_DTYPE_F32 ? 0 : 1, cp, m.sh_conv.cout);
}

// a ScalarHead-shaped branch over the tower output x: hc 1x1 filters, hs hidden units, the outputs to `out`
inline kz::ScalarHeadArgs kz_engine::scalar_head_args(const ScalarBranch &s, const void *x, int batch, int hc, int hs, float *out) const {
    return kz::ScalarHeadArgs{x, cp, batch, model->h * model->w, model->channels, hc, hs, s.w0, s.b0, s.w1, s.b1, s.w2, s.b2, out, nullptr, 0, s.w1t};
}

inline int kz_engine::run_heads(const Pass &p, int batch, float *d_scalars, float *d_policy) {
    if (plan.heads || plan.tower == Tower::dense_net) return 0;  // written by the tower launch
    const Model &m = *model;
    const int hw = m.h * m.w, M = batch * hw;
    const void *x = act[tower_out];
    if (plan.att_heads) {  // ScalarHead + AttentionPolicyHead in one launch
        kz::AttHeadsArgs a{};
        a.x = x; a.ldx = cp; a.batch = batch; a.channels = m.channels; a.q = m.policy_query_channels;
        a.hc = m.sh_conv.cout; a.hs = m.sh_fc0.out; a.policy_len = m.policy_len;
        a.weights = wts->pol.ah_w; a.bias = wts->pol.ah_bias;
        a.w1 = wts->sh.w1; a.b1 = wts->sh.b1; a.w2 = wts->sh.w2; a.b2 = wts->sh.b2;
        a.flat_to_att = wts->pol.flat_to_att; a.scalars = d_scalars; a.policy = d_policy;
        a.nonfinite_flag = p.nf_flag; a.epoch = p.nf_epoch;
        return launch(p, "kz_att_heads_f16", [&] { kz::launch_att_heads(a, p.stream); });
    }
    {
        kz::ScalarHeadArgs a = scalar_head_args(wts->sh, x, batch, m.sh_conv.cout, m.sh_fc0.out, d_scalars);
        a.nonfinite_flag = p.nf_flag; a.epoch = p.nf_epoch;
        // ConvPolicyHead's extra moves read the same tower output: one pass for both (post_act.py:63-67)
        if (extra_in_scalar_head()) {
            a.extra = m.policy_extra_moves;
            a.w0x = wts->pol.w0x; a.pe_bc = wts->pol.pe_bc; a.pe_wl = wts->pol.pe_wl; a.pe_bl = wts->pol.pe_bl;
            a.policy = d_policy; a.policy_len = m.policy_len; a.policy_offset = m.policy_conv_channels * hw;
        }
        if (launch(p, "kz_scalar_head", [&] { kz::launch_scalar_head(dtype, a, p.stream); })) return 1;
    }
    switch (m.policy_kind) {
        case kz::POLICY_ATAXX_CONV:
        case kz::POLICY_CONV: {
            const int pc = m.policy_conv_channels;
            const DevConv &c0 = wts->pol.conv0;
            if (m.policy_kind == kz::POLICY_CONV && c0.sw && cp >= c0.cin_p &&
                kz::conv1x1_policy_epilogue_supported(c0.cin_p, c0.cout_p, c0.cout, pc)) {
                // Conv1x1 C->C + ReLU + Conv1x1 C->1 in one launch: the hidden layer never goes to memory
                kz::Conv1x1SplitArgs c{};
                c.split = split16();
                c.x = x; c.ldx = cp; c.weights = c0.sw; c.bias = c0.b; c.y = nullptr; c.ldy = 0;
                c.M = M; c.cin_p = c0.cin_p; c.cout_p = c0.cout_p; c.relu = 1;
                c.group = hw; c.src_group = hw; c.src_off = 0;
                c.pw1 = wts->pol.w1; c.pb1 = wts->pol.b1; c.policy = d_policy; c.policy_len = m.policy_len; c.hw = hw;
                if (launch(p, "kz_conv1x1_split", [&] { kz::launch_conv1x1_split(c, p.stream); })) return 1;
            } else {
                if (conv(p, c0, x, cp, head0, c0.cout_p, M, 1, nullptr, false, m.h, m.w, hw, hw, 0)) return 1;
                kz::PolicyConvArgs a{head0, c0.cout_p, batch, hw, m.channels, pc, wts->pol.w1, wts->pol.b1,
                                     d_policy, m.policy_len, m.policy_kind == kz::POLICY_ATAXX_CONV ? 1 : 0};
                if (launch(p, "kz_policy_conv", [&] { kz::launch_policy_conv(dtype, a, p.stream); })) return 1;
            }
            if (m.policy_kind == kz::POLICY_CONV && m.policy_extra_moves && !extra_in_scalar_head()) {
                kz::PolicyExtraArgs e{x, cp, batch, hw, m.channels, m.policy_extra_moves, wts->pol.pe_wc, wts->pol.pe_bc,
                                      wts->pol.pe_wl, wts->pol.pe_bl, d_policy, m.policy_len, pc * hw};
                if (launch(p, "kz_policy_extra", [&] { kz::launch_policy_extra(dtype, e, p.stream); })) return 1;
            }
            break;
        }
        case kz::POLICY_ARIMAA: {
            // ArimaaPolicyHead (post_act.py:144-173): policy = concat(scalar(common) [1 + 6], flatten(bulk(common)) [4 * hw])
            const DevConv &c0 = wts->pol.conv0;
            if (conv(p, c0, x, cp, head0, c0.cout_p, M, 1, nullptr, false, m.h, m.w, hw, hw, 0)) return 1;
            kz::PolicyConvArgs a{head0, c0.cout_p, batch, hw, m.channels, 4, wts->pol.w1, wts->pol.b1,
                                 d_policy + 7, m.policy_len, 0};  // (the four planes start behind the seven scalars)
            if (launch(p, "kz_policy_conv", [&] { kz::launch_policy_conv(dtype, a, p.stream); })) return 1;
            // the scalar branch has the ScalarHead's shape: the same kernel, seven outputs into the policy rows
            kz::ScalarHeadArgs sa = scalar_head_args(wts->pol.arimaa, x, batch, m.arimaa_hidden_channels, m.arimaa_hidden_size, d_policy);
            sa.n_out = 7;
            sa.out_ld = m.policy_len;
            if (launch(p, "kz_scalar_head", [&] { kz::launch_scalar_head(dtype, sa, p.stream); })) return 1;
            break;
        }
        case kz::POLICY_ATTENTION: {
            // bulk = conv_bulk(common) on all 64 squares; under = conv_under(common[:, :, 7, None, :]) on the
            // 8 squares of rank index 7 (post_act.py:128-129): source rows 56..63 of each board
            if (conv(p, wts->pol.bulk, x, cp, head0, wts->pol.bulk.cout_p, M, 0, nullptr, false, m.h, m.w, hw, hw, 0))
                return 1;
            if (conv(p, wts->pol.under, x, cp, head1, wts->pol.under.cout_p, batch * 8, 0, nullptr, false, 1, 8, 8, hw, 56))
                return 1;
            kz::AttentionArgs a{head0, head1, wts->pol.bulk.cout_p, wts->pol.under.cout_p, batch,
                                m.policy_query_channels, wts->pol.flat_to_att, d_policy, m.policy_len};
            if (launch(p, "kz_attention_gather", [&] { kz::launch_attention(dtype, a, p.stream); })) return 1;
            break;
        }
        case kz::POLICY_NONE: break;
        case kz::POLICY_DENSE: {
            const void *flat = x;
            int flat_ld = hw * cp;
            if (m.dense_hidden_channels) {
                if (conv(p, wts->pol.conv0, x, cp, head0, wts->pol.conv0.cout_p, M, 1, nullptr, false, m.h, m.w, hw, hw, 0))
                    return 1;
                flat = head0;
                flat_ld = hw * wts->pol.conv0.cout_p;
            }
            // Flatten + Linear: one GEMM row per board
            if (m.dense_hidden_size) {
                if (conv(p, wts->pol.fc0, flat, flat_ld, head1, wts->pol.fc0.cout_p, batch, 1, nullptr, false, 1, 1, 1, 1, 0))
                    return 1;
                if (conv(p, wts->pol.fc1, head1, wts->pol.fc0.cout_p, nullptr, 0, batch, 0, nullptr, false, 1, 1, 1, 1, 0,
                         d_policy, m.policy_len))
                    return 1;
            } else {
                if (conv(p, wts->pol.fc1, flat, flat_ld, nullptr, 0, batch, 0, nullptr, false, 1, 1, 1, 1, 0, d_policy,
                         m.policy_len))
                    return 1;
            }
            break;
        }
    }
    return 0;
}

// dec (plan.heads only): the launch ends in decode_output and writes dec->values / dec->probs
inline int kz_engine::forward_packed(const Pass &p, const kz::PackedBoards &in, int batch, void *d_sout, void *d_pol, const kz::DecodeArgs *dec) {
    const Model &m = *model;
    if (encodes_boards(plan)) {
        if (run_tower(p, batch, (float *)d_sout, (float *)d_pol, &in, dec)) return 1;
        return run_heads(p, batch, (float *)d_sout, (float *)d_pol);
    }
    if (launch(p, "kz_encode_packed", [&] { kz::launch_encode_packed(dtype, in, batch, m.h * m.w, x_in, cin_p, p.stream); })) return 1;
    if (run_tower(p, batch, (float *)d_sout, (float *)d_pol)) return 1;
    return run_heads(p, batch, (float *)d_sout, (float *)d_pol);
}

inline int kz_engine::forward_dense(const Pass &p, const void *d_nchw, int batch, void *d_sout, void *d_pol) {
    const Model &m = *model;
    if (launch(p, "kz_encode_dense", [&] { kz::launch_encode_dense(dtype, (const float *)d_nchw, batch, m.c_in, m.h * m.w, x_in, cin_p, p.stream); }))
        return 1;
    if (run_tower(p, batch, (float *)d_sout, (float *)d_pol)) return 1;
    return run_heads(p, batch, (float *)d_sout, (float *)d_pol);
}
