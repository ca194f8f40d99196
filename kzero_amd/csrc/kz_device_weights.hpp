// kz_device_weights.hpp — device weights: the packed weight streams of the kernels a plan names.  DeviceWeights::build(model, spec)
// sees of the plan its WeightsSpec (kz_plan.hpp: weights_spec) and nothing else, and all engines with the same WeightsKey — the
// model, the device, the dtype and that spec — share one reference-counted DeviceWeights.  build packs on the host — one pack_*
// function per tower family and per head, none with a HIP call: each hands host buffers, with the members that get their device
// addresses, to a Staged list — and sends every list through the one upload.  Part of kz_engine.hip's translation unit
// (included inside its anonymous namespace, after kz_engine_util.hpp and kz_plan.hpp).
#pragma once

struct DevConv {  // packed for kz_conv_igemm: [k*k][cout_p][cin_p] in T, bias f32 [cout_p]
    void *w = nullptr;
    float *b = nullptr;
    int cin_p = 0, cout_p = 0, cout = 0, k = 1;
    void *bw = nullptr;  // instead of w: packed for kz_board_conv_f16 (3x3, f16, channels % 64 == 0)
    bool bw2 = false;    // ... packed for kz_board_conv2_f16 (two Go-size boards per workgroup)
    void *bws = nullptr; // instead of w: (hi, lo) pairs packed for kz_board_conv_split16 (3x3, split arithmetic)
    void *sw = nullptr;  // in addition to w: (hi, lo) f16 pairs for kz_conv1x1_split (1x1 head convolutions, split16)
};

// the matrices of a ScalarHead-shaped branch (Conv1x1 + ReLU, Flatten, Linear + ReLU, Linear), as the model has them:
// w0 [hc][C] is the OIHW 1x1 conv as is, w1 keeps the channel-major flatten order; w1t is w1 transposed, [inputs][outputs]
struct ScalarBranch {
    float *w0 = nullptr, *b0 = nullptr, *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr, *w1t = nullptr;
};

// the host side of device buffers to be: each one's bytes — a vector handed over, or one of the model's own — and the member
// that gets the device address
struct Staged {
    struct Buf {
        std::shared_ptr<void> own;  // (empty: src is the model's)
        const void *src;
        size_t bytes;
        void **dst;
    };
    std::vector<Buf> bufs;
    template <class T, class P> T *take(std::vector<T> v, P **dst) {
        auto h = std::make_shared<std::vector<T>>(std::move(v));
        bufs.push_back({h, h->data(), h->size() * sizeof(T), (void **)dst});
        return h->data();
    }
    template <class T, class P> void ref(const std::vector<T> &v, P **dst) { bufs.push_back({nullptr, v.data(), v.size() * sizeof(T), (void **)dst}); }
};

struct DeviceWeights {
    int device = 0, dtype = 0;
    std::vector<void *> allocs;
    bool split16 = false;  // split_arithmetic(spec.tower): pack_conv packs the 1x1 head convolutions in (hi, lo) pairs

    // the per-layer towers (board_conv_f16, board_conv_split16, conv_igemm): one DevConv per convolution
    std::vector<DevConv> tower;
    int stem_cin_p = 0;  // != 0: the stem goes through the board-tile kernel and wants encoded rows of this many channels
    bool stem_split = false;  // split16 per layer: the stem too goes through kz_board_conv_split16 (<= 32 input planes)
    bool conv2 = false;  // (experiment build, spec.conv2) the board-tile layers go through kz_board_conv2_f16 ...
    int *bc_rowmap = nullptr, bc_n_halo = 0;  // ... with its tile-row map and halo-row list
    unsigned short *bc_halo = nullptr;
    // board_conv_i8 (kz_board_conv_i8.hip): per convolution the packed stream (the stem's in f16, the block convolutions' in
    // int8), bias and multiplier 2^(e_in + f_oc) over the widened channels [C8], and 2^-e of the site its int8 image is stored
    // at; the final BatchNorm over [C8]
    struct I8Conv {
        void *w = nullptr;
        float *bias = nullptr, *mult = nullptr;
        float qscale = 1.0f;
    };
    std::vector<I8Conv> i8conv;
    float *post8_scale = nullptr, *post8_shift = nullptr;
    int c8 = 0;
    // every tower but the dense network: the final BatchNorm, [round_up(C, 32)]
    float *post_scale = nullptr, *post_shift = nullptr;
    // the one-launch ResTowers.  resident_f32, resident_split16, resident_f16g, resident_bf16g: w32 and bias (and small where
    // the stream carries the conv heads); resident_f16: w_stem, w_tower and bias; att_idx where it carries the attention heads;
    // resident_i8: w32, bias, mult and qscale (and small, in f16, where the stream carries the conv heads)
    struct {
        void *w32 = nullptr;  // one packed weight stream: exact f32, split f16 pairs, plain f16 or bf16; f16 stem + int8 blocks
        float *mult = nullptr;    // resident_i8: [1 + 2·depth][C], 2^(e_in + f_oc) per block convolution and output channel
        float *qscale = nullptr;  // resident_i8: [2·depth], 2^-e_s per quantised range site
        void *w_stem = nullptr, *w_tower = nullptr;
        float *bias = nullptr;  // [1 + 2·depth (+ head rows)][C]
        float *small = nullptr;  // the fused conv heads' small 1x1 convolutions (tower32_pack_small_weights, or in f16)
        int32_t *att_idx = nullptr;
    } res;
    // AttentionTower.  att_valu: the model's own matrices in f32 (expand, embedding, layers); att_mfma: expand16 and layers16
    // in the engine's arithmetic, embedding
    struct {
        float *expand = nullptr, *embedding = nullptr, *layers = nullptr;
        void *expand16 = nullptr, *layers16 = nullptr;
    } att;
    // DenseNetwork (dense_net: the whole network, nothing else is set)
    struct {
        float *w_in = nullptr, *b_in = nullptr, *blocks = nullptr, *sf = nullptr, *tf = nullptr, *w_out = nullptr, *b_out = nullptr;
    } dn;
    // scalar head: every plan but dense_net
    ScalarBranch sh;
    // policy head, by the model's policy kind: every plan but dense_net and resident_f16 with the heads in its stream
    struct {
        DevConv conv0;                                 // conv / ataxx_conv / arimaa / dense: the hidden conv
        float *w1 = nullptr, *b1 = nullptr;            // conv / ataxx_conv / arimaa: the last 1x1 conv
        float *pe_wc = nullptr, *pe_bc = nullptr, *pe_wl = nullptr, *pe_bl = nullptr;  // conv with extra moves (seq_extra)
        float *w0x = nullptr;  // ... [hc + 1][C]: the scalar head's 1x1 filters followed by the extra-move filter
        ScalarBranch arimaa;   // ArimaaPolicyHead's scalar branch (post_act.py:155-162)
        DevConv bulk, under;   // attention, three separate launches
        void *ah_w = nullptr;  // attention, spec.att_heads: ScalarHead + AttentionPolicyHead in one f16 launch (kz_att_heads.hip)
        float *ah_bias = nullptr;
        int32_t *flat_to_att = nullptr;  // attention, either way
        DevConv fc0, fc1;      // dense
    } pol;

    ~DeviceWeights() {
        (void)hipSetDevice(device);
        for (void *p : allocs) (void)hipFree(p);
    }

    int upload(Staged &st) {
        for (auto &b : st.bufs) {
            HIP_TRY(hipMalloc(b.dst, b.bytes ? b.bytes : 16));
            allocs.push_back(*b.dst);
            if (b.bytes) HIP_TRY(hipMemcpy(*b.dst, b.src, b.bytes, hipMemcpyHostToDevice));
        }
        st.bufs.clear();
        return 0;
    }

    // ---- helpers of the pack functions ----
    // f32 values -> T, the engine's element type
    void put_matrix(std::vector<float> v, void **dst, Staged &st) {
        if (dtype == KZ_DTYPE_F32) {
            st.take(std::move(v), dst);
        } else {
            std::vector<uint16_t> p(v.size());
            for (size_t i = 0; i < v.size(); i++) p[i] = f32_to_f16_bits(v[i]);
            st.take(std::move(p), dst);
        }
    }
    // a DevConv's bias, zero padded to cout_p
    void put_padded_bias(const std::vector<float> &b, DevConv &d, Staged &st) {
        std::vector<float> p(d.cout_p, 0.0f);
        std::copy(b.begin(), b.begin() + d.cout, p.begin());
        st.take(std::move(p), &d.b);
    }
    // the one-launch towers' bias table -> res.bias: [1 + 2·depth + head_rows][C], the head rows zero but for the first where
    // `head` is given.  Returns the first head row
    float *put_bias_rows(const Model &m, int head_rows, const Conv *head, Staged &st) {
        const int C = m.channels, n = 1 + 2 * m.depth;
        std::vector<float> bias((size_t)(n + head_rows) * C);
        for (int l = 0; l < n; l++) std::copy(m.tower[l].b.begin(), m.tower[l].b.begin() + C, bias.begin() + (size_t)l * C);
        if (head) std::copy(head->b.begin(), head->b.begin() + C, bias.begin() + (size_t)n * C);
        return st.take(std::move(bias), &res.bias) + (size_t)n * C;
    }
    // the fused attention heads' gather table -> res.att_idx: rows of 88 logits in rows of 96
    void put_att_idx(const Model &m, Staged &st) {
        std::vector<int32_t> idx(m.flat_to_att.size());
        for (size_t i = 0; i < idx.size(); i++) idx[i] = (m.flat_to_att[i] / 88) * 96 + m.flat_to_att[i] % 88;
        st.take(std::move(idx), &res.att_idx);
    }
    // the fused conv heads' small 1x1 convolutions in f32 -> res.small
    void put_small_weights(const Model &m, Staged &st) {
        std::vector<float> small(kz::tower32_small_weight_elems(m.channels));
        kz::tower32_pack_small_weights(m.sh_conv.w.data(), m.sh_conv.cout, m.policy_extra_moves ? m.p_extra_conv.w.data() : nullptr,
                                       m.p_conv1.w.data(), m.policy_conv_channels, m.channels, small.data());
        st.take(std::move(small), &res.small);
    }
    // OIHW 3x3 weights with the input planes padded with zero weights to cin: the stem in one chunk of a board-tile kernel
    static const float *pad_cin(const Conv &cv, int cin, std::vector<float> &padded) {
        if (cin == cv.cin) return cv.w.data();
        padded.assign((size_t)cv.cout * cin * 9, 0.0f);
        for (int o = 0; o < cv.cout; o++)
            std::copy(cv.w.begin() + (size_t)o * cv.cin * 9, cv.w.begin() + (size_t)(o + 1) * cv.cin * 9, padded.begin() + (size_t)o * cin * 9);
        return padded.data();
    }
    void pack_scalar_branch(const Conv &conv, const Linear &fc0, const Linear &fc1, ScalarBranch &s, Staged &st) {
        st.ref(conv.w, &s.w0); st.ref(conv.b, &s.b0); st.ref(fc0.w, &s.w1); st.ref(fc0.b, &s.b1); st.ref(fc1.w, &s.w2); st.ref(fc1.b, &s.b2);
        std::vector<float> wt((size_t)fc0.in * fc0.out);
        for (int o = 0; o < fc0.out; o++)
            for (int i = 0; i < fc0.in; i++) wt[(size_t)i * fc0.out + o] = fc0.w[(size_t)o * fc0.in + i];
        st.take(std::move(wt), &s.w1t);
    }

    // ---- one convolution or Linear for the per-layer kernels ----
    // 3x3 tower conv for the board-tile kernel (kz_board_conv.hip), plain f16 or — split — in (hi, lo) pairs.  cin_pad: the
    // stem's few input planes padded to the kernel's chunk of 64 (split: 32) channels
    void pack_board_conv(const Conv &cv, DevConv &d, bool split, int cin_pad, Staged &st) {
        d.k = 3;
        d.cout = d.cout_p = cv.cout;
        const int cin = d.cin_p = cin_pad ? cin_pad : cv.cin;
        std::vector<float> padded;
        const float *w = pad_cin(cv, cin, padded);
        std::vector<uint16_t> packed(split ? kz::board_conv_split_weight_elems(cin, cv.cout) : kz::board_conv_weight_elems(cin, cv.cout));
        if (split) kz::board_conv_split_pack_weights(w, cv.cout, cin, packed.data());
#ifdef KZ_EXPERIMENTS
        else if ((d.bw2 = conv2)) kz::board_conv2_pack_weights(w, cv.cout, cin, packed.data());
#endif
        else kz::board_conv_pack_weights(w, cv.cout, cin, packed.data());
        st.take(std::move(packed), split ? &d.bws : &d.bw);
        st.ref(cv.b, &d.b);
    }
    // OIHW conv -> [tap][cout_p][cin_p]; tap = ky*k + kx
    void pack_conv(const Conv &cv, DevConv &d, Staged &st) {
        d.k = cv.k;
        d.cout = cv.cout;
        d.cin_p = round_up(cv.cin, 32);
        d.cout_p = round_up(cv.cout, 32);
        const int taps = cv.k * cv.k;
        std::vector<float> flat((size_t)taps * d.cout_p * d.cin_p, 0.0f);
        for (int o = 0; o < cv.cout; o++)
            for (int i = 0; i < cv.cin; i++)
                for (int t = 0; t < taps; t++)
                    flat[((size_t)t * d.cout_p + o) * d.cin_p + i] = cv.w[((size_t)o * cv.cin + i) * taps + t];
        put_matrix(std::move(flat), &d.w, st);
        // 1x1 head convolutions: the tiled GEMM of kz_tower_split.hip in split arithmetic (split16) or plain f16
        if ((split16 || dtype == KZ_DTYPE_F16) && cv.k == 1 && kz::conv1x1_split_supported(d.cin_p, d.cout_p)) {
            std::vector<uint16_t> packed(kz::conv1x1_split_weight_elems(d.cin_p, d.cout_p, split16));
            kz::conv1x1_split_pack_weights(cv.w.data(), cv.cout, cv.cin, d.cout_p, d.cin_p, split16, packed.data());
            st.take(std::move(packed), &d.sw);
        }
        put_padded_bias(cv.b, d, st);
    }
    // nn.Linear as a 1x1 "convolution" over one row per board.  hw != 0: over a channel-major flatten of [ch][hw] (index
    // c*hw + p) applied to NHWC rows [hw][ch_p] — the input dimension re-indexed to p*ch_p + c
    void pack_linear(const Linear &l, DevConv &d, Staged &st, int ch = 0, int hw = 0, int ch_p = 0) {
        d.k = 1;
        d.cout = l.out;
        d.cout_p = round_up(l.out, 32);
        d.cin_p = hw ? hw * ch_p : round_up(l.in, 32);
        std::vector<float> flat((size_t)d.cout_p * d.cin_p, 0.0f);
        for (int o = 0; o < l.out; o++) {
            if (!hw) std::copy(l.w.begin() + (size_t)o * l.in, l.w.begin() + (size_t)(o + 1) * l.in, flat.begin() + (size_t)o * d.cin_p);
            for (int c = 0; c < ch; c++)
                for (int p = 0; p < hw; p++) flat[(size_t)o * d.cin_p + (size_t)p * ch_p + c] = l.w[(size_t)o * l.in + (size_t)c * hw + p];
        }
        put_matrix(std::move(flat), &d.w, st);
        put_padded_bias(l.b, d, st);
    }

    // ---- the tower families ----
    void pack_dense_network(const Model &m, Staged &st) {
        // dn_in's columns from the channel-major flatten (c * hw + p) to the encoded rows' order (p * cin_p + c)
        const int C = m.channels, hw = m.h * m.w, cin_p = round_up(m.c_in, 32), n_in = hw * cin_p;
        std::vector<float> w_in((size_t)C * n_in, 0.0f);
        for (int o = 0; o < C; o++)
            for (int c = 0; c < m.c_in; c++)
                for (int p = 0; p < hw; p++) w_in[(size_t)o * n_in + (size_t)p * cin_p + c] = m.dn_in.w[(size_t)o * m.dn_in.in + (size_t)c * hw + p];
        std::vector<float> blocks;
        blocks.reserve(kz::dense_network_block_elems(C) * m.dn_blocks.size());
        for (auto &b : m.dn_blocks)
            for (const std::vector<float> *v : {&b.sa, &b.ta, &b.la.w, &b.la.b, &b.sb, &b.tb, &b.lb.w, &b.lb.b}) blocks.insert(blocks.end(), v->begin(), v->end());
        st.take(std::move(w_in), &dn.w_in); st.ref(m.dn_in.b, &dn.b_in); st.take(std::move(blocks), &dn.blocks);
        st.ref(m.dn_sf, &dn.sf); st.ref(m.dn_tf, &dn.tf); st.ref(m.dn_out.w, &dn.w_out); st.ref(m.dn_out.b, &dn.b_out);
    }
    void pack_post(const Model &m, Staged &st) {
        const int cp = round_up(m.channels, 32);
        std::vector<float> ps(cp, 1.0f), pt(cp, 0.0f);
        std::copy(m.final_scale.begin(), m.final_scale.begin() + m.channels, ps.begin());
        std::copy(m.final_shift.begin(), m.final_shift.begin() + m.channels, pt.begin());
        st.take(std::move(ps), &post_scale);
        st.take(std::move(pt), &post_shift);
    }
    void pack_att_mfma(const Model &m, Staged &st) {
        const int C = m.channels, cin_p = round_up(m.c_in, 32);
        const bool f32 = dtype == KZ_DTYPE_F32;
        const size_t esz = f32 ? 4 : 2;
        std::vector<char> ex(kz::att_tower16_expand_elems(C, cin_p) * esz);
        kz::att_tower16_pack_expand(m.att_expand.data(), C, m.c_in, cin_p, f32, ex.data());
        const size_t per = kz::att_tower16_layer_elems(C, m.att_dff) * esz;
        std::vector<char> all(per * m.att_layers.size());
        for (size_t l = 0; l < m.att_layers.size(); l++)
            kz::att_tower16_pack_layer(m.att_layers[l].qkv.data(), m.att_layers[l].out.data(), m.att_layers[l].ff0.data(),
                                       m.att_layers[l].ff1.data(), C, m.att_dff, m.att_alpha, f32, all.data() + per * l);
        st.take(std::move(ex), &att.expand16);
        st.take(std::move(all), &att.layers16);
        st.ref(m.att_embedding, &att.embedding);
    }
    void pack_att_valu(const Model &m, Staged &st) {
        std::vector<float> all;
        all.reserve(kz::att_tower_layer_elems(m.channels, m.att_heads, m.att_dk, m.att_dv, m.att_dff) * m.att_layers.size());
        for (auto &l : m.att_layers)
            for (const std::vector<float> *v : {&l.qkv, &l.out, &l.ff0, &l.ff1}) all.insert(all.end(), v->begin(), v->end());
        st.ref(m.att_expand, &att.expand);
        st.ref(m.att_embedding, &att.embedding);
        st.take(std::move(all), &att.layers);
    }
    // resident_split16, resident_f16g, resident_bf16g: f16 fragments — (hi, lo) pairs for split16, bf16 elements for bf16g — in
    // fragment order: 9 * ceil(c_in / 32) stem k-steps, then 9*C/32 per convolution, then the heads the stream carries — the
    // attention heads' five passes and bias rows (the split launch only), or the conv heads (Ataxx, Go 9x9): the policy head's
    // hidden layer as one more pass, the small convolutions beside the stream
    void pack_pairs(const Model &m, const WeightsSpec &s, Staged &st) {
        const int C = m.channels, hw = m.h * m.w;
        const bool bf16 = s.tower == Tower::resident_bf16g;
        const bool conv_heads = s.heads == StreamHeads::conv, heads = s.heads == StreamHeads::attention;
        const size_t tower_elems = kz::tower_split_weight_elems(C, m.depth, m.c_in, split16);
        std::vector<uint16_t> packed(tower_elems + (heads ? kz::tower_split_heads_weight_elems() : 0) +
                                     (conv_heads ? kz::tower_split_conv_heads_weight_elems(C, split16) : 0));
        const size_t step_elems = (size_t)(split16 ? 2 : 1) * C * 32, stem_elems = kz::tower_split_stem_elems(C, m.c_in, split16),
                     layer_elems = (size_t)9 * (C / 32) * step_elems;
        kz::tower_split_pack_weights(m.tower[0].w.data(), C, m.c_in, hw, true, split16, packed.data(), bf16);
        for (int l = 0; l < 2 * m.depth; l++)
            kz::tower_split_pack_weights(m.tower[1 + l].w.data(), C, C, hw, false, split16, packed.data() + stem_elems + layer_elems * l, bf16);
        float *head_bias = put_bias_rows(m, heads ? 5 : conv_heads ? 1 : 0, conv_heads ? &m.p_conv0 : nullptr, st);
        if (conv_heads) {
            kz::tower_split_pack_conv_heads(m.p_conv0.w.data(), C, split16, packed.data() + tower_elems, bf16);
            if (!split16 && !bf16) {  // the plain-f16 launch runs the two small convolutions as f16 MFMAs
                std::vector<uint16_t> small(kz::tower_split_small_weight16_elems(C));
                kz::tower_split_pack_small_weights16(m.sh_conv.w.data(), m.sh_conv.cout, m.policy_extra_moves ? m.p_extra_conv.w.data() : nullptr,
                                                     m.p_conv1.w.data(), m.policy_conv_channels, C, small.data());
                st.take(std::move(small), &res.small);
            } else {
                put_small_weights(m, st);
            }
        }
        if (heads) {
            kz::tower_split_pack_heads(m.p_bulk.w.data(), m.p_bulk.b.data(), m.p_under.w.data(), m.p_under.b.data(), packed.data() + tower_elems, head_bias);
            put_att_idx(m, st);
        }
        st.take(std::move(packed), &res.w32);
    }
    // resident_i8 (a calibrated model: m.i8_exp): the stem's k-steps as f16 fragments, the block convolutions' as int8 fragments
    // — 16 B per lane, 64 channels per k-step —, one f32 multiplier table beside the bias table.  The weight exponent of a
    // (block convolution, output channel) is f = ceil(log2(max |w[oc]| / 127)) on the folded weights, wq = rne(w · 2^-f); an
    // all-zero filter (a widened channel) gets f = 0.  Every scale is a power of two: exact to apply.
    // With the conv heads in the stream ("tower_resident_i8+heads"): the policy head's hidden layer as one more pass of C/32 f16
    // k-steps behind the tower's (a k-step is C * 64 bytes in either element), its bias as one more bias row, and the plain-f16
    // launch's small convolutions beside the stream; without them the stream is byte for byte what it was.
    void pack_i8(const Model &m, const WeightsSpec &s, Staged &st) {
        const int C = m.channels, hw = m.h * m.w, layers = 2 * m.depth;
        const bool conv_heads = s.heads == StreamHeads::conv;
        const size_t stem_bytes = kz::tower_split_stem_elems(C, m.c_in, false) * 2, layer_bytes = kz::tower_i8_layer_bytes(C);
        const size_t tower_bytes = stem_bytes + layer_bytes * layers;
        std::vector<uint8_t> packed(tower_bytes + (conv_heads ? kz::tower_split_conv_heads_weight_elems(C, false) * 2 : 0));
        kz::tower_split_pack_weights(m.tower[0].w.data(), C, m.c_in, hw, true, false, reinterpret_cast<uint16_t *>(packed.data()));
        std::vector<float> mult((size_t)(1 + layers) * C, 1.0f), qscale(layers);
        std::vector<int8_t> wq((size_t)C * C * 9);
        for (int l = 1; l <= layers; l++) {
            const std::vector<float> &w = m.tower[l].w;
            const int e_in = m.i8_exp[l - 1];
            for (int oc = 0; oc < C; oc++) {
                const float *row = w.data() + (size_t)oc * C * 9;
                float top = 0.0f;
                for (int i = 0; i < C * 9; i++) top = std::max(top, std::fabs(row[i]));
                const int f = top > 0.0f ? kz::i8_exponent(top) : 0;
                for (int i = 0; i < C * 9; i++) wq[(size_t)oc * C * 9 + i] = (int8_t)std::nearbyint(std::ldexp((double)row[i], -f));
                mult[(size_t)l * C + oc] = std::ldexp(1.0f, e_in + f);  // (|e_in| <= I8_EXP_MAX, f32 weights: a normal f32 or, far out, 0 / inf like the weight itself)
            }
            kz::tower_i8_pack_weights(wq.data(), C, reinterpret_cast<int8_t *>(packed.data() + stem_bytes + layer_bytes * (l - 1)));
        }
        for (int s = 0; s < layers; s++) qscale[s] = std::ldexp(1.0f, -m.i8_exp[s]);
        put_bias_rows(m, conv_heads ? 1 : 0, conv_heads ? &m.p_conv0 : nullptr, st);
        if (conv_heads) {
            kz::tower_split_pack_conv_heads(m.p_conv0.w.data(), C, false, reinterpret_cast<uint16_t *>(packed.data() + tower_bytes));
            std::vector<uint16_t> small(kz::tower_split_small_weight16_elems(C));
            kz::tower_split_pack_small_weights16(m.sh_conv.w.data(), m.sh_conv.cout, m.policy_extra_moves ? m.p_extra_conv.w.data() : nullptr,
                                                 m.p_conv1.w.data(), m.policy_conv_channels, C, small.data());
            st.take(std::move(small), &res.small);
        }
        st.take(std::move(mult), &res.mult);
        st.take(std::move(qscale), &res.qscale);
        st.take(std::move(packed), &res.w32);
    }
    // board_conv_i8 (a calibrated model), one convolution per call like pack_per_layer: the tower widened to C8 channels by
    // all-zero filters.  i = 0: the stem for the f16 board-tile instance, its input planes padded to chunks of 64 (the encode
    // kernel then writes rows of that many channels); i >= 1: wq and f_oc exactly as pack_i8 computes them, the multiplier
    // table 2^(e_in + f_oc) beside the bias (1 and 0 on a widened channel)
    void pack_board_i8(const Model &m, size_t i, Staged &st) {
        const int C = m.channels, C8 = kz::board_conv_i8_channels(C), layers = 2 * m.depth;
        if (i == 0) {
            i8conv.resize(m.tower.size());
            c8 = C8;
            std::vector<float> ps(C8, 1.0f), pt(C8, 0.0f);
            std::copy(m.final_scale.begin(), m.final_scale.begin() + C, ps.begin());
            std::copy(m.final_shift.begin(), m.final_shift.begin() + C, pt.begin());
            st.take(std::move(ps), &post8_scale);
            st.take(std::move(pt), &post8_shift);
        }
        I8Conv &d = i8conv[i];
        const Conv &cv = m.tower[i];
        std::vector<float> bias(C8, 0.0f), mult(C8, 1.0f);
        std::copy(cv.b.begin(), cv.b.begin() + C, bias.begin());
        if (i == 0) {
            const int cin = stem_cin_p = round_up(cv.cin, 64);
            std::vector<float> w((size_t)C8 * cin * 9, 0.0f);
            for (int o = 0; o < C; o++)
                std::copy(cv.w.begin() + (size_t)o * cv.cin * 9, cv.w.begin() + (size_t)(o + 1) * cv.cin * 9, w.begin() + (size_t)o * cin * 9);
            std::vector<uint16_t> packed(kz::board_conv_weight_elems(cin, C8));
            kz::board_conv_pack_weights(w.data(), C8, cin, packed.data());
            st.take(std::move(packed), &d.w);
        } else {
            const int e_in = m.i8_exp[i - 1];
            std::vector<int8_t> wq((size_t)C * C * 9);
            for (int oc = 0; oc < C; oc++) {
                const float *row = cv.w.data() + (size_t)oc * C * 9;
                float top = 0.0f;
                for (int k = 0; k < C * 9; k++) top = std::max(top, std::fabs(row[k]));
                const int f = top > 0.0f ? kz::i8_exponent(top) : 0;
                for (int k = 0; k < C * 9; k++) wq[(size_t)oc * C * 9 + k] = (int8_t)std::nearbyint(std::ldexp((double)row[k], -f));
                mult[oc] = std::ldexp(1.0f, e_in + f);
            }
            std::vector<int8_t> packed(kz::board_conv_i8_weight_bytes(C8, C8));
            kz::board_conv_i8_pack_weights(wq.data(), C, C, C8, C8, packed.data());
            st.take(std::move(packed), &d.w);
        }
        if ((int)i < layers) d.qscale = std::ldexp(1.0f, -m.i8_exp[i]);  // (the last range site is not quantised)
        st.take(std::move(bias), &d.bias);
        st.take(std::move(mult), &d.mult);
    }
    // resident_f32.  (The conv policy head's first 1x1 conv rides at the end of the stream whenever the launch can fuse the
    // heads — weights_spec says so; a launch without heads never reads it)
    void pack_resident_f32(const Model &m, const WeightsSpec &s, Staged &st) {
        const int C = m.channels;
        const bool heads32 = s.heads == StreamHeads::conv;
        const size_t tower_elems = kz::tower32_weight_elems(m.c_in, C, m.depth);
        std::vector<float> packed(tower_elems + (heads32 ? kz::tower32_heads_weight_elems(C) : 0) + kz::tower32_weight_pad_elems(C), 0.0f);
        const size_t stem_elems = (size_t)9 * ((m.c_in + 15) / 16) * 16 * C, layer_elems = (size_t)9 * C * C;
        kz::tower32_pack_weights(m.tower[0].w.data(), C, m.c_in, true, packed.data());
        for (int l = 0; l < 2 * m.depth; l++)
            kz::tower32_pack_weights(m.tower[1 + l].w.data(), C, C, false, packed.data() + stem_elems + layer_elems * l);
        put_bias_rows(m, heads32 ? 1 : 0, heads32 ? &m.p_conv0 : nullptr, st);
        if (heads32) {
            kz::tower32_pack_head_weights(m.p_conv0.w.data(), C, packed.data() + tower_elems);
            put_small_weights(m, st);
        }
        st.take(std::move(packed), &res.w32);
    }
    // resident_f16 (256 channels): the stem, then the layers — tap by tap for the experiment build's four-board launch — with
    // the attention heads' five passes and bias rows behind them where the stream carries the heads
    void pack_resident_f16(const Model &m, const WeightsSpec &s, Staged &st) {
        const int C = m.channels, cin_p = round_up(m.c_in, 32);
        const bool heads = s.heads == StreamHeads::attention;
        const size_t stem_elems = (size_t)9 * 256 * cin_p, layer_elems = (size_t)9 * 256 * 256;
        const size_t head_elems = heads ? kz::tower_heads_weight_elems() : 0;
        std::vector<uint16_t> stem(stem_elems), rest(layer_elems * 2 * m.depth + head_elems + kz::tower_weight_pad_elems());
        kz::tower_pack_weights(m.tower[0].w.data(), C, m.c_in, cin_p, stem.data());
        for (int l = 0; l < 2 * m.depth; l++) kz::tower_pack_weights(m.tower[1 + l].w.data(), C, C, 256, rest.data() + layer_elems * l, s.nb4);
        float *head_bias = put_bias_rows(m, heads ? 5 : 0, nullptr, st);
        if (heads) {
            kz::tower_pack_heads(m.p_bulk.w.data(), m.p_bulk.b.data(), m.p_under.w.data(), m.p_under.b.data(),
                                 rest.data() + layer_elems * 2 * m.depth, head_bias);
            put_att_idx(m, st);
        }
        st.take(std::move(stem), &res.w_stem);
        st.take(std::move(rest), &res.w_tower);
    }
    // per layer — board_conv_f16 / board_conv_split16 / conv_igemm (the stem and layers no board-tile kernel takes) —, one
    // convolution per call: build uploads each before the next is packed, so the host never holds more than one layer's stream
    void pack_per_layer(const Model &m, const WeightsSpec &s, size_t i, Staged &st) {
        const bool on = s.tower == Tower::board_conv_f16, use_board_split = s.tower == Tower::board_conv_split16;
        if (i == 0) {
            tower.resize(m.tower.size());
#ifdef KZ_EXPERIMENTS
            conv2 = s.conv2;  // (the second organisation measured 26.2k against 33.5k evals/s on Go-19 40x256)
            if (conv2) {  // its tile-row map and halo-row list (the product kernel needs no tables)
                std::vector<int> rowmap;
                std::vector<unsigned short> halo;
                kz::board_conv2_tables(m.h, m.w, rowmap, halo);
                bc_n_halo = (int)halo.size();
                st.take(std::move(rowmap), &bc_rowmap);
                st.take(std::move(halo), &bc_halo);
            }
#endif
        }
        // the stem joins the board-tile family with its input planes padded to one 64-channel chunk (the encode
        // kernel then writes 64-channel rows): a quarter of a tower layer's work instead of an implicit GEMM
        const bool stem64 = on && i == 0 && !conv2 && m.tower[0].cin <= 64 && m.tower[0].k == 3 &&
                            kz::board_conv_supported(dtype, m.h, m.w, 64, m.tower[0].cout);
        const bool board = on && kz::board_conv_supported(dtype, m.h, m.w, m.tower[i].cin, m.tower[i].cout);
        // the split stem through the same kernel: its input planes as one 32-channel chunk of (hi, lo) rows — an eighth of a
        // 256-channel layer's work instead of an exact-f32 implicit GEMM and a splitting pass (which a stem of more planes stays)
        const bool stem32 = use_board_split && i == 0 && m.tower[0].cin <= 32 && m.tower[0].k == 3;
        if (stem32) stem_split = true;
        if (stem64) stem_cin_p = 64;
        if (stem32 || (use_board_split && i >= 1)) pack_board_conv(m.tower[i], tower[i], true, stem32 ? 32 : 0, st);
        else if (stem64 || board) pack_board_conv(m.tower[i], tower[i], false, stem64 ? 64 : 0, st);
        else pack_conv(m.tower[i], tower[i], st);
    }

    // ---- the policy heads behind a materialised tower output ----
    // conv / ataxx_conv, and ArimaaPolicyHead's bulk (the same pair with four planes): the hidden conv, the last 1x1 conv
    void pack_policy_conv_pair(const Model &m, Staged &st) {
        pack_conv(m.p_conv0, pol.conv0, st);
        st.ref(m.p_conv1.w, &pol.w1);
        st.ref(m.p_conv1.b, &pol.b1);
    }
    void pack_policy_conv(const Model &m, Staged &st) {
        pack_policy_conv_pair(m, st);
        if (!m.policy_extra_moves) return;
        st.ref(m.p_extra_conv.w, &pol.pe_wc); st.ref(m.p_extra_conv.b, &pol.pe_bc); st.ref(m.p_extra_fc.w, &pol.pe_wl); st.ref(m.p_extra_fc.b, &pol.pe_bl);
        if (m.sh_conv.cout == 4 && m.p_extra_conv.cout == 1 && m.p_extra_conv.cin == m.sh_conv.cin) {
            std::vector<float> w0x(m.sh_conv.w);  // [4][C] ...
            w0x.insert(w0x.end(), m.p_extra_conv.w.begin(), m.p_extra_conv.w.end());  // ... + [1][C]
            st.take(std::move(w0x), &pol.w0x);
        }
    }
    void pack_policy_arimaa(const Model &m, Staged &st) {  // the scalar branch: a second ScalarHead
        pack_policy_conv_pair(m, st);
        pack_scalar_branch(m.pa_conv, m.pa_fc0, m.pa_fc1, pol.arimaa, st);
    }
    void pack_policy_attention(const Model &m, const WeightsSpec &s, Staged &st) {
        if (s.att_heads) {
            const int Q = m.policy_query_channels;
            std::vector<uint16_t> packed(kz::att_heads_weight_elems(m.channels, Q));
            std::vector<float> bias((size_t)5 * Q + 16);
            kz::att_heads_pack(m.p_bulk.w.data(), m.p_bulk.b.data(), m.p_under.w.data(), m.p_under.b.data(), m.sh_conv.w.data(),
                               m.sh_conv.b.data(), m.channels, Q, m.sh_conv.cout, packed.data(), bias.data());
            st.take(std::move(packed), &pol.ah_w);
            st.take(std::move(bias), &pol.ah_bias);
        } else {
            pack_conv(m.p_bulk, pol.bulk, st);
            pack_conv(m.p_under, pol.under, st);
        }
        st.ref(m.flat_to_att, &pol.flat_to_att);
    }
    void pack_policy_dense(const Model &m, Staged &st) {
        const int hw = m.h * m.w;
        int ch = m.channels, ch_p = round_up(m.channels, 32);
        if (m.dense_hidden_channels) {
            pack_conv(m.p_conv0, pol.conv0, st);
            ch = m.dense_hidden_channels;
            ch_p = pol.conv0.cout_p;
        }
        if (m.dense_hidden_size) {
            pack_linear(m.p_fc0, pol.fc0, st, ch, hw, ch_p);
            pack_linear(m.p_fc1, pol.fc1, st);
        } else {
            pack_linear(m.p_fc1, pol.fc1, st, ch, hw, ch_p);
        }
    }

    // (device and dtype set before: the engine's, KZ_DTYPE_F32 for split arithmetic)
    int build(const Model &m, const WeightsSpec &s) {
        split16 = split_arithmetic(s.tower);
        HIP_TRY(hipSetDevice(device));
        Staged st;
        if (s.tower == Tower::dense_net) {
            pack_dense_network(m, st);
            return upload(st);
        }
        pack_post(m, st);
        switch (s.tower) {
            case Tower::att_mfma: pack_att_mfma(m, st); break;
            case Tower::att_valu: pack_att_valu(m, st); break;
            case Tower::resident_split16:
            case Tower::resident_f16g:
            case Tower::resident_bf16g: pack_pairs(m, s, st); break;
            case Tower::resident_i8: pack_i8(m, s, st); break;
            case Tower::resident_f32: pack_resident_f32(m, s, st); break;
            case Tower::resident_f16: pack_resident_f16(m, s, st); break;
            case Tower::board_conv_i8:
                for (size_t i = 0; i < m.tower.size(); i++) {
                    pack_board_i8(m, i, st);
                    if (upload(st)) return 1;
                }
                break;
            default:
                for (size_t i = 0; i < m.tower.size(); i++) {
                    pack_per_layer(m, s, i, st);
                    if (upload(st)) return 1;
                }
        }
        pack_scalar_branch(m.sh_conv, m.sh_fc0, m.sh_fc1, sh, st);
        if (upload(st)) return 1;
        if (s.tower == Tower::resident_f16 && s.heads != StreamHeads::none) return 0;  // the policy head lives in the tower's weight stream
        switch (m.policy_kind) {
            case kz::POLICY_ATAXX_CONV:
            case kz::POLICY_CONV: pack_policy_conv(m, st); break;
            case kz::POLICY_ARIMAA: pack_policy_arimaa(m, st); break;
            case kz::POLICY_ATTENTION: pack_policy_attention(m, s, st); break;
            case kz::POLICY_DENSE: pack_policy_dense(m, st); break;
            case kz::POLICY_NONE: break;
        }
        return upload(st);
    }
};

// engines with equal keys share one DeviceWeights: the spec is all that build sees of a plan
struct WeightsKey {
    const Model *model;
    int device, dtype;
    WeightsSpec spec;
    bool operator<(const WeightsKey &o) const { return std::tie(model, device, dtype, spec) < std::tie(o.model, o.device, o.dtype, o.spec); }
};
std::mutex g_cache_mutex;
std::map<WeightsKey, std::weak_ptr<DeviceWeights>> g_cache;
