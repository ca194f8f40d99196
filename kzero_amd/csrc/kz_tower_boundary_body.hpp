// kz_tower_boundary_body.hpp — included INSIDE kz_tower_resident's body (kz_tower.hip), behind conv_3x3_lines: the 3x3
// layer of the line-tile instances (two boards per workgroup, not PREV, not TAP) with a shorter serial section between
// two layers.  The k-steps, their order, the weight stream, the fragment reads and the ring are conv_3x3_lines'; every sum
// is the same sum in the same order.  Inside a k-step the MFMAs walk the tiles in the boustrophedon of
// kz_tower_mfma_order.hpp (conv_3x3_lines: ascending), which changes fewer operand registers from one MFMA to the next and
// no sum: every accumulator still receives one MFMA per k-step.  What else differs is work that stood between two layers
// with the matrix pipe idle:
//  * no accumulator initialisation.  The first MFMA into an accumulator takes the bias registers as its C operand: in the
//    first super-step (dx = -1, chunk 0) tiles 1..7 at dy = -1 and tile 0 at dy = 0.  bias + a*b in one instruction is what
//    acc = bias; acc = a*b + acc computes.  The coming layer's bias is fetched behind the dy = +1 k-step of that
//    super-step, once the last MFMA that reads this layer's has issued.
//  * conv A's ReLU on the packed f16 bits (kz_tower_boundary.hpp, relu_f16_bits): one packed max per two values.
//  * the coming layer's first row addresses are the "next dx" addresses of dx = +1, which had no successor: Tl carries
//    them across the boundary.  (The fragment prefetch of the last super-step, which nothing uses, re-reads this layer's
//    own rows as before: the coming layer's image is being written.)
// The three dx are unrolled: the first and the last super-step differ from the other 22, and a layer's k-loop has to stay
// ONE basic block.  With a scalar branch on dx around a super-step — one branch was enough — the register allocator
// parked live values in accumulator registers and scratch on both sides of it (352 to 900 bytes of scratch, 100 to 150
// v_accvgpr moves in the k-loop: tools/layer_boundary_isa.py).  Unrolled there is neither, the row addresses of a dx are
// compile-time taps, and the compiler itself starts reading finished accumulators under the last MFMAs.
constexpr bool LEAN = L::LINE_TILES && !PREV && !TAP;
// the three tap rows' tile ranges, as the MFMA order takes them
constexpr kz_mfma_order::Rows ORDER_ROWS{3, {tile_lo(-1), tile_lo(0), tile_lo(1)}, {tile_hi(-1), tile_hi(0), tile_hi(1)}, {-1, 0, 1}};
int Tl[MT];  // this lane's fragment rows of the coming layer's first dx (dx = -1)
if constexpr (LEAN) tap_rows(0, -1, L::X_OFF, Tl);

// acc = bias + sum over the nine taps and all 256 input channels of W * image(src_off).  next_off: the image the coming
// layer reads; next_bias_row: its row of the bias table.
auto conv_3x3_lean = [&](int src_off, int next_off, int next_bias_row) __attribute__((always_inline)) {
    static_assert(!L::LINE_TILES || MT == 8, "one tile per board line");
    int Tn[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) bf[0][mt] = *reinterpret_cast<const h16x8 *>(lds + Tl[mt]);
    static_for<0, 3>([&](auto dx_tag) __attribute__((always_inline)) {
        constexpr int dx = decltype(dx_tag)::value - 1;
        static_for<0, 8>([&](auto ch_tag) __attribute__((always_inline)) {
            constexpr int ch = decltype(ch_tag)::value, cur = ch & 1, nxt = cur ^ 1;
            constexpr bool FIRST = dx == -1 && ch == 0, LAST = dx == 1 && ch == 7;  // of the layer's 24 super-steps
            // once per dx: the next dx's row addresses — after dx = +1 the coming layer's first ones
            if constexpr (ch == 0) tap_rows(0, dx < 1 ? dx + 1 : -1, dx < 1 ? src_off : next_off, Tn);
            // next super-step's line fragments: LDS -> registers
#ifndef KZ_TW_NO_DSREAD  // (timing experiments: a build without the fragment reads)
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
                bf[nxt][mt] = *reinterpret_cast<const h16x8 *>(lds + (ch < 7 ? Tl[mt] + (ch + 1) * 16 : LAST ? Tl[mt] : Tn[mt]));
#endif
            static_for<0, 3>([&](auto i_tag) __attribute__((always_inline)) {
                constexpr int i = decltype(i_tag)::value, dy = i - 1, stage = (ch * 3 + i) & (PF - 1);
                constexpr int lo = tile_lo(dy), hi = tile_hi(dy), nt_ = hi - lo;
                // this k-step's weight fragments were loaded PF k-steps ago
                h16x8 af[4];
                ring_take(stage, af);
                // (output-channel tile outermost: the weight fragment is held for all pixel tiles; the tiles in the
                // boustrophedon of kz_tower_mfma_order.hpp, so that one MFMA and the next differ in one operand register)
                static_for<0, 4 * nt_>([&](auto j_tag) __attribute__((always_inline)) {
                    constexpr kz_mfma_order::Pos p = kz_mfma_order::at(ORDER_ROWS, i, decltype(j_tag)::value);
                    constexpr int nt = p.nt, mt = p.mt;
                    constexpr bool opens = FIRST && (mt == 0 ? i == 1 : i == 0);  // the accumulator's first MFMA, wherever it stands in the order
                    if constexpr (LEAN)  // (the other instances never call this layer; their tiles are not lines)
                        acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[nt], bf[cur][mt + dy], opens ? bias_next[nt] : acc[nt][mt], 0, 0, 0);
                });
                constexpr int n_bias = FIRST && i == 2 ? 4 : 0;
                if constexpr (n_bias != 0) fetch_bias(next_bias_row);
                // issue order: the 4 ring refills (and the 4 bias loads) behind the first MFMAs of the k-step; the 8
                // fragment reads behind the next MFMAs of the super-step's first k-step; once per dx, the row addresses
                // two behind each MFMA
#pragma unroll
                for (int j = 0; j < 4 + n_bias; j++) {
                    __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(SG_VMEM_READ, 1, 0);
                }
                constexpr int nr = i == 0 ? MT : 0;
#pragma unroll
                for (int j = 0; j < MT; j++) {
                    if (j < nr) {
                        __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(SG_DS_READ, 1, 0);
                    }
                }
                constexpr int n_free = 4 * nt_ - (nr + 4 + n_bias), n_alu = ch == 0 && i == 0 ? n_free : 0;
                static_assert(n_free >= 0, "every memory instruction of a k-step has an MFMA to ride behind");
#pragma unroll
                for (int j = 0; j < 4 * MT; j++) {
                    if (j < n_alu) {
                        __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(SG_VALU | SG_SALU, 2, 0);
                    }
                }
                __builtin_amdgcn_sched_group_barrier(SG_MFMA, n_free - n_alu, 0);
                __builtin_amdgcn_sched_barrier(0);
                g++;
            });
        });
#pragma unroll
        for (int mt = 0; mt < MT; mt++) Tl[mt] = Tn[mt];
    });
};

// epilogue of a lean layer: ReLU; [+ residual X]; [final BN]; -> f16 -> LDS image at dst_off.  Flags are compile-time.
auto epilogue_lean = [&](int dst_off, auto residual, auto post) __attribute__((always_inline)) {
    if constexpr (decltype(residual)::value) {
        epilogue(dst_off, YES, residual, post);
    } else {
        // conv A: convert, then ReLU on the packed f16 bits — the same bits as relu4 and then the conversion
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        typedef h16 h16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int nt = 0; nt < 4; nt++)
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const f32x4 v = acc[nt][mt];
                const h16x2 lo = __builtin_convertvector(f32x2{v[0], v[1]}, h16x2), hi = __builtin_convertvector(f32x2{v[2], v[3]}, h16x2);
                const boundary::s16x2 rl = boundary::relu_f16_bits(__builtin_bit_cast(boundary::s16x2, lo));
                const boundary::s16x2 rh = boundary::relu_f16_bits(__builtin_bit_cast(boundary::s16x2, hi));
                *reinterpret_cast<uint2 *>(lds + dst_off + epi_base + mt * L::TS + nt * 32) =
                    make_uint2(__builtin_bit_cast(unsigned, rl), __builtin_bit_cast(unsigned, rh));
            }
    }
};
