/*
 * kz_hip.h — C ABI of the MI355X-native self-play NN executor for kZero.
 *
 * This is the drop-in boundary: the entry points a Rust `HipNetwork<B, M>: Network<B>` binds over FFI in place
 * of the kn-cuda-eval `CudaExecutor` used by `CudaNetwork` (rust/kz-core/src/network/cudnn.rs:18-88).  Plain
 * pointers and sizes only.  Every function returns 0 on success and non-zero on error; `kz_last_error()` gives
 * the message (the reference panics on every error: `unwrap()` cudnn.rs:70,78, `assert!` :58 — the Rust shim
 * turns a non-zero return into a panic to keep that behaviour).
 *
 * Threading contract (mirrors the reference): `kz_model` is immutable and may be shared by any number of threads
 * and devices (it is the `Arc<Graph>` sent to every executor, rust/kz-selfplay/src/server/commander.rs:36-45).
 * `kz_engine` is NOT thread-safe: one per executor thread (`evaluate_batch(&mut self)`, kz-core/src/network/mod.rs:56),
 * created on that thread like `CudaNetwork::new` in `handle_new_graph` (kz-selfplay/src/server/executor.rs:320-342).
 * Engines of one model on one device share a single uploaded copy of the weights.
 */
#ifndef KZ_HIP_H
#define KZ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KZ_DTYPE_F32 0 /* f32 storage, exact-f32 MFMA: the <=1e-4 parity path (the reference is f32 only, cudnn.rs:73) */
#define KZ_DTYPE_F16 1 /* f16 storage, f32 accumulate: the throughput path.  RANGE: activations are stored as f16, so a
                          residual stream beyond +-65504 overflows; the overflow is DETECTED, not saturated: the call that
                          returns the batch (kz_engine_eval_*, kz_engine_wait*, or kz_engine_synchronize after the
                          device-resident entry points) fails with a "non-finite activation" message and the caller
                          should evaluate that network with KZ_DTYPE_F32 — or, board by board and inside the engine, turn on
                          kz_engine_set_range_fallback (below).  The same limit and the same check apply to
                          KZ_DTYPE_F32_SPLIT16 (its (hi, lo) pairs are f16 too) */
#define KZ_DTYPE_F32_SPLIT16 2 /* f32 tensors and the same <=1e-4 parity as KZ_DTYPE_F32, but the tower's products run on
                                  the f16 matrix cores: every activation and weight as a (hi, lo) f16 pair, three MFMAs per
                                  product, f32 accumulate.  One launch per batch for 192 / 256 tower channels on <= 64
                                  squares or 64 / 128 channels on <= 96 squares, with no more input planes than tower
                                  channels; one launch per layer otherwise (Go 19x19, wider towers: channels a multiple
                                  of 64, max_batch * squares * channels * 4 bytes < 2 GiB).  A tower whose channel count
                                  is no multiple of 64 (48, 96, 160 ... up to 512) runs widened to the next one by
                                  all-zero filters (same outputs).  kz_engine_create fails for the rest — a tower without
                                  blocks, more than 512 channels in no multiple of 64 — and kz_model_supports_dtype
                                  tells.  Everything outside the tower is the KZ_DTYPE_F32 path */
#define KZ_DTYPE_BF16 3 /* f32 tensors at every boundary, like KZ_DTYPE_F32_SPLIT16 — the f32 engine with the tower's launch
                           exchanged —, the tower in bf16: products bf16 x bf16 with f32 accumulation
                           (v_mfma_f32_16x16x32_bf16, the rate of the f16 instruction), the residual stream and the mid
                           activation stored as bf16 (round to nearest even), bias, ReLU, residual add and the final BN in
                           f32.  RANGE: bf16 has f32's exponent, so a residual stream beyond +-65504 — every ResBlock adds a
                           non-negative term that nothing re-normalises before the final BN — does NOT overflow here: no
                           status to watch, no sibling engine; the non-finite check stays and can only fire on an f32
                           overflow.  PRECISION: 8 significant bits where f16 has 11 (the contract: README, "which number is
                           which arithmetic"; kz_engine_set_audit measures it on a network's own positions).  One launch
                           per batch ("tower_resident_bf16g", "+heads" with the conv policy heads at 128 / 256 channels,
                           their tail in exact f32) for the shapes of the plain-f16 one-launch tower: 64 .. 512 tower
                           channels in a multiple of 64 (others widened, as above) on the small boards — 256 / 320
                           channels on <= 96 squares, 384 / 512 on <= 64, 192 on <= 176, 128 on <= 208, 64 on <= 96.
                           kz_engine_create fails, and kz_model_supports_dtype says 0, for Go 19x19 and any other shape
                           that runs per layer, AttentionTower networks, DenseNetworks and a tower without blocks.
                           Everything outside the tower is the KZ_DTYPE_F32 path */
#define KZ_DTYPE_INT8 4 /* f16 tensors at every boundary — the f16 engine with the tower's launch exchanged —, the tower's block
                           convolutions on the i8 matrix cores (v_mfma_i32_16x16x64_i8: the f16 instruction's 16 bytes per
                           lane, twice its k): int8 activations and weights, exact i32 sums, one power-of-two scale per range
                           site and per (block convolution, output channel).  Only a CALIBRATED model runs it
                           (kz_model_quantize_int8 below, which also states the arithmetic to the bit).  The stem and the
                           residual stream stay f16 (RANGE: the +-65504 limit and the non-finite check of KZ_DTYPE_F16,
                           unchanged; saturation of a quantised image at +-127 steps is silent by design — counted per
                           site by kz_model_int8_error_profile), bias, ReLU,
                           residual add and the final BN are f32.  PRECISION: 7 bits and a sign per stored activation where
                           f16 has 11 (README, "which number is which arithmetic"; kz_engine_set_audit measures it on a
                           network's own positions).  One launch for the tower ("tower_resident_i8"; no "+heads": the f16
                           engine's head kernels follow it) at 256 tower channels on <= 64 squares (two 8x8 boards per
                           workgroup when max_batch gives 128 such workgroups) and 128 channels on <= 96 squares (there
                           wide tiles chosen per launch from its batch: two 8x8 / two 9x9 / four 7x7 / eight 5x5 boards per
                           workgroup in a batch of 256 such workgroups, else the narrow tiles — measured thresholds,
                           DESIGN.md 6.2.3; the bits do not depend on it; kz_model_launch_geometry says which); a
                           channel count in between runs widened to the next multiple of 64, as above: 193 .. 255 as 256,
                           65 .. 127 as 128.  64 channels or fewer, 129 .. 192 and more than 256 have no int8 kernel.  kz_engine_create fails, and kz_model_supports_dtype says 0, for
                           an uncalibrated model, every other shape, AttentionTower networks, DenseNetworks and a tower
                           without blocks; the message says whether the calibration or the kernel is missing, and to a model
                           that carries no calibration dtype 4 is, first of all, an unknown dtype.  It reads
                           none of the environment switches.  kz_model_tower_taps, _taps_path and kz_model_error_profile
                           refuse it: kz_model_int8_taps, _taps_path and kz_model_int8_error_profile are its own */
#define KZ_DTYPE_INT8_HEADS 5 /* KZ_DTYPE_INT8's tower, bit for bit, with the heads inside its launch where the launch can carry
                                 them: ScalarHead, ConvPolicyHead or AtaxxConvPolicyHead and decode_output run behind the last
                                 block in f16, on the f16 values the tower holds — the plain-f16 launch's tail
                                 ("tower_resident_f16g+heads"), so the heads' bits are that tail's, not those of the separate
                                 head kernels behind dtype 4.  "tower_resident_i8+heads": ONE launch per batch, zero-copy slots
                                 on two streams like every "+heads" plan.  That is 128 tower channels (65 .. 127 widened) on
                                 <= 96 squares and 256 (193 .. 255 widened) on <= 64, a conv policy head with <= 32 planes, a
                                 scalar head of <= 32 channels (one less with extra moves) and <= 256 hidden units, at most
                                 four boards per workgroup on the narrow tiles, the tail's floats within 16 KB of LDS.  Where
                                 the narrow tiles carry the heads, the launch also takes wide tiles at 128 channels, per
                                 launch from its batch: dtype 4's levels from 128 such workgroups, and sixteen tiles — three 9x9
                                 or four 8x8 boards, a level that exists with the heads inside only — from 342, up to the widest
                                 level whose tail still fits (at most four boards; at sixteen tiles 9,728 B are left for the
                                 tail: three Go 9x9 boards with the default scalar head fit, four 8x8 boards stay at two per
                                 workgroup, 5x5 boards at the narrow tiles' four);
                                 always ONE 8x8 board per workgroup at 256 channels.  kz_model_launch_geometry says which.
                                 Everywhere else —
                                 attention or dense policy heads, more boards per workgroup — dtype 5 is EXACTLY dtype 4's
                                 plan: same path name, same launches, same bits; a caller can always pass 5.
                                 kz_model_supports_dtype(m, 5) == kz_model_supports_dtype(m, 4) for every model; the refusals
                                 are dtype 4's with "dtype 5" in them (an uncalibrated model: first of all an unknown dtype 5);
                                 it reads none of the environment switches; the taps and the error profile refuse it */
/* (6 and 7 are not dtypes: they stay unknown, like every other value not defined here.) */
#define KZ_DTYPE_INT8_ANY 8 /* KZ_DTYPE_INT8_HEADS with a per-layer int8 kernel behind it.  On a calibrated ResTower model it is
                               EXACTLY dtype 5's plan wherever dtype 5 has one: same path name, same launches, same bits.  Where
                               dtype 5 refuses the shape — Go 19x19 and 13x13, Go 9x9 at 256 channels, a tower above 256
                               channels, of 64 or fewer, of 129 .. 192 — it is "board_conv_i8": one launch per layer
                               (kz_board_conv_i8, the board-tile kernel of "board_conv_f16" on v_mfma_i32_16x16x64_i8), the
                               arithmetic of "int8 calibration" below to the bit, which is stated per convolution and does not
                               depend on the geometry.  The stem is the f16 board-tile stem with two stores from one f32 v:
                               f16(v) for the residual stream and quant(v, e_0).  That plan takes a tower with at least one
                               block on a board of 2 .. 32 squares a side that fits a workgroup of the board-tile kernels (24
                               tiles of 16 squares, the halo image within its LDS) and at most 512 channels after widening; it
                               has NO minimum of workgroups (the alternative is a refusal, not another kernel).  CHANNELS: the
                               int8 images hold the tower widened to the next multiple of 128, a chunk of the kernel, by
                               all-zero filters (f = 0, bias 0; every widened channel of every image is 0, same outputs): 64
                               or fewer run as 128, 129 .. 256 as 256, up to 512; the f16 stream keeps the f16 engine's rows.
                               The tensors around the tower are f16, as for dtype 4: the f16 engine's encode, head kernels
                               and decode run around it (no "+heads"), and symmetries, per-board status, range fallback, audit
                               and every entry point work as for dtype 4.  Refusals are dtype 4's with "dtype 8" in them (an
                               uncalibrated model: first of all an unknown dtype 8); it reads none of the environment
                               switches; the taps and the error profile refuse it.  kz_model_launch_geometry reports the
                               per-layer plan's workgroups (64 output channels of the widened tower per workgroup).  SPEED, measured against the
                               f16 engine of the same build in the same process (README, "which number is which arithmetic";
                               profiles/int8_board_rate.json): Go 19x19 40x256 at batch 512 1.51 of f16 through the decoded
                               entries, Go 9x9 16x256 at 2048 1.37 — at 7 bits and a sign per stored activation */

#define KZ_POLICY_ATAXX_CONV 0 /* AtaxxConvPolicyHead, python/lib/model/post_act.py:91-112 */
#define KZ_POLICY_CONV 1       /* ConvPolicyHead,      post_act.py:54-88 */
#define KZ_POLICY_ATTENTION 2  /* AttentionPolicyHead, post_act.py:115-141 */
#define KZ_POLICY_DENSE 3      /* DensePolicyHead,     post_act.py:26-51 */
#define KZ_POLICY_ARIMAA 4     /* ArimaaPolicyHead,    post_act.py:144-173 (the server's arimaa-split game, server.rs:174) */
#define KZ_POLICY_NONE 5       /* no PredictionHeads: a DenseNetwork (python/lib/model/simple.py:7-33), one Linear yields scalars and policy */

typedef struct kz_model kz_model;
typedef struct kz_engine kz_engine;

/* What `check_graph_shapes` compares against the mapper (rust/kz-core/src/network/common.rs:165-198):
 * input [BATCH, input_channels, board_h, board_w] with input_channels = scalar + bool planes (scalars first,
 * kz-core/src/mapping/mod.rs:40-63); outputs [BATCH, 5] and [BATCH, policy_len]. */
typedef struct kz_model_info {
    int32_t input_channels;
    int32_t board_h;
    int32_t board_w;
    int32_t input_scalar_channels; /* -1: unknown (ONNX loaded without the split) */
    int32_t input_bool_channels;   /* -1: unknown */
    int32_t policy_len;
    int32_t tower_depth;
    int32_t tower_channels;
    int32_t policy_kind;
    int32_t bits_bytes;     /* ceil(input_bool_channels * h * w / 8): BitBuffer storage per board (bit_buffer.rs:8-14); -1: unknown */
    int64_t param_count;
    double flops_per_eval;  /* direct-convolution FLOPs (2 per MAC), heads included: the roofline numerator */
} kz_model_info;

/* Thread-local message of the last failing call on this thread. */
const char *kz_last_error(void);

/* Replaces CudaDevice::all() (rust/kz-selfplay/src/server/server.rs:48-52). */
int kz_device_count(int *count);
/* PCI bus id of `device` as a NUL-terminated string ("0000:c1:00.0"): lets a launcher that starts one process per GPU
 * prove that its ranks sit on distinct devices (bench.py reports the set). */
int kz_device_pci_bus_id(int device, char *buf, size_t len);

/* ---- model: replaces load_graph_from_onnx_path + optimize_graph (server_alphazero.rs:126-128) ----
 * Accepts the KZMODEL1 container (kzero_amd/model_file.py); Conv+BN folding happens here. */
int kz_model_load(const char *path, kz_model **out);
int kz_model_load_memory(const void *blob, size_t len, kz_model **out);
/* The ONNX file the trainer already writes (python/lib/save_onnx.py:60-122: opset 10, input "input", outputs "scalars"
 * and "policy"), i.e. what `Command::NewNetwork(path)` carries (kz-selfplay/src/server/protocol.rs:36).  The graph does
 * not say how many of its input planes are broadcast scalars: pass the mapper's `input_scalar_count()`
 * (kz-core/src/mapping/mod.rs:21).  kz_model_load/_memory also accept ONNX, with the split unknown: such a model
 * serves kz_engine_eval_dense only and the packed entry points fail with a message. */
int kz_model_load_onnx(const char *path, int input_scalar_channels, kz_model **out);
int kz_model_load_onnx_memory(const void *blob, size_t len, int input_scalar_channels, kz_model **out);
void kz_model_free(kz_model *model);
int kz_model_get_info(const kz_model *model, kz_model_info *out);

/* ---- engine: replaces CudaNetwork::new(mapper, &graph, max_batch_size, device) (cudnn.rs:29-43) ---- */
int kz_engine_create(const kz_model *model, int device, int max_batch, int dtype, kz_engine **out);
void kz_engine_destroy(kz_engine *engine);
/* 1 when kz_engine_create would accept `dtype` for this model, 0 when not (KZ_DTYPE_F32_SPLIT16 has shape limits,
 * see above), negative on a null/unknown argument.  Lets a host pick "the fastest path with <= 1e-4 parity":
 * KZ_DTYPE_F32_SPLIT16 where supported, else KZ_DTYPE_F32. */
int kz_model_supports_dtype(const kz_model *model, int dtype);
/* What kz_engine_create(model, any device, max_batch, dtype) WOULD choose, without touching a GPU: the tower path (the
 * names kz_engine_tower_path documents) and the kernel launches one packed-input batch takes.  Pure host logic over the
 * kernels' support predicates — DESIGN.md §5.0 prints its path table from it and a CPU test holds it to a committed
 * copy.  Fails (non-zero, kz_last_error) exactly when kz_engine_create would refuse the dtype for this model. */
typedef struct kz_path_plan {
    char tower_path[48];
    int32_t launches_per_batch;
    int32_t reserved[3];
} kz_path_plan;
int kz_model_plan(const kz_model *model, int max_batch, int dtype, kz_path_plan *out);
int kz_engine_max_batch(const kz_engine *engine); /* Network::max_batch_size, network/mod.rs:53 */

/* ---- synchronous evaluation: replaces CudaNetwork::evaluate_batch's encode + executor.evaluate (cudnn.rs:55-82) ----
 * Only `batch` rows are computed and written (the reference NaN-pads to max_batch and discards, cudnn.rs:65,75-82).
 * batch must be in [0, max_batch]; batch == 0 is a no-op.  Caller owns all buffers; nothing is retained. */

/* Bit-compatible with CudaExecutor::evaluate: dense f32 NCHW [batch, C, H, W] as built by encode_input_full. */
int kz_engine_eval_dense(kz_engine *engine, const float *input_nchw, int batch, float *scalars_out /* [batch,5] */,
                         float *policy_out /* [batch,policy_len] */);

/* Packed input, the GPU does encode_input_full: `bits` = BitBuffer storage per board (LSB-first,
 * bit_buffer.rs:73-75), bits_stride bytes apart; `scalars_in` [batch, input_scalar_channels] as appended by
 * InputMapper::encode_input (mapping/mod.rs:37). */
int kz_engine_eval_packed(kz_engine *engine, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                          int batch, float *scalars_out, float *policy_out);

/* Packed input AND decoded output: decode_output (rust/kz-core/src/network/common.rs:16-100) runs on the GPU, so only
 * the decoded values and the probabilities of the available moves cross PCIe (~0.2 KB instead of 7.5 KB per chess eval).
 * move_offsets [batch+1] (CSR; move_offsets[0] == 0) and move_indices [move_offsets[batch]] list, per board and in
 * available_moves() order, `PolicyMapper::move_to_index(board, mv)` (kz-core/src/mapping/mod.rs:74) of every available
 * move; a finished board has an empty range (common.rs:77 `map_or(vec![], ..)`).
 * values_out [batch,5] = value (tanh), win, draw, loss (softmax), moves_left; probs_out parallel to move_indices.
 * Fails — where the reference asserts `sum > 0.0` (common.rs:110) — when a softmax sum is not strictly positive. */
int kz_engine_eval_packed_decoded(kz_engine *engine, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                                  int batch, const int64_t *move_offsets, const int32_t *move_indices,
                                  float *values_out, float *probs_out);

/* ---- asynchronous pair: several batches in flight per executor thread (replaces gpu_threads_per_device blocking
 * threads, rust/Readme.md:51).  slot in [0, KZ_ENGINE_SLOTS).  Inputs are copied to the slot's pinned staging before
 * submit returns; outputs are written to the caller's buffers by kz_engine_wait.  On the one-launch chess path the slots
 * alternate over two streams (a batch of 256 is half a chip of workgroups: two launches run side by side, the next launch
 * of a stream starts when the previous one ends) and the launch reads and writes the pinned staging directly, so no copy
 * operation sits between launches: keep all four slots submitted to keep both halves of the chip busy. */
#define KZ_ENGINE_SLOTS 4
int kz_engine_submit_packed(kz_engine *engine, int slot, const uint8_t *bits, size_t bits_stride,
                            const float *scalars_in, int batch);
int kz_engine_wait(kz_engine *engine, int slot, float *scalars_out, float *policy_out);
/* Same wait without the copy: *scalars_out [batch*5] and *policy_out [batch*policy_len] point into the slot's pinned
 * staging (library-owned) and stay valid until the next kz_engine_submit_packed on that slot or kz_engine_destroy —
 * the lifetime of the `&[DTensor]` the reference's executor hands out until its next call (cudnn.rs:73-82).  Saves a
 * 1.9 MB host copy per chess batch of 256 on the executor thread. */
int kz_engine_wait_view(kz_engine *engine, int slot, const float **scalars_out, const float **policy_out);
/* The asynchronous pair with decode_output on the device (kz_engine_eval_packed_decoded split in two): submit takes
 * the CSR move lists of the batch (move_offsets [batch+1], move_indices = move_to_index of every available move),
 * wait hands out views of the slot's pinned staging — values [batch*5] (value, win, draw, loss, moves_left) and the
 * probabilities parallel to move_indices — valid until the next submit on that slot.  0.2 KB instead of 7.5 KB per
 * chess evaluation cross PCIe and the executor thread does no softmax. */
int kz_engine_submit_packed_decoded(kz_engine *engine, int slot, const uint8_t *bits, size_t bits_stride,
                                    const float *scalars_in, int batch, const int64_t *move_offsets,
                                    const int32_t *move_indices);
int kz_engine_wait_decoded(kz_engine *engine, int slot, const float **values_out, const float **probs_out);

/* ---- board symmetries inside the launch: `RandomSymmetryNetwork` (rust/kz-core/src/network/symmetry.rs:18-68,126-148;
 * the `eval_random_symmetries` start-up setting) without host work.  The reference maps the board, evaluates the mapped
 * board and reads each move's probability at the index of its mapped move; here the launch does both permutations, so the
 * caller passes the ORIGINAL board's bits and the move_to_index of the ORIGINAL board's moves, plus one symmetry id per board.
 * The library does not know the game: a symmetry is a row of each of two tables,
 *   square_src [n_sym][board_h * board_w]: the mapped board's bool planes at square s are the board's own at
 *                                          square_src[id][s] (a permutation of the squares; scalar planes do not move),
 *   policy_map [n_sym][policy_len]:        the move with policy index i has index policy_map[id][i] on the mapped board;
 *                                          -1 = the mapped board has no such move.
 * kz_engine_set_symmetries checks 1 <= n_sym <= 255, that every square_src row is a permutation and every policy_map entry
 * is in [-1, policy_len), and copies the tables to the device.  It may be called again (other tables) while no batch is in
 * flight, on an engine of any path and dtype.  host/symmetry.hpp builds the D4 tables of Ataxx and Go.
 * The _sym entries are kz_engine_eval_packed_decoded / kz_engine_submit_packed_decoded with `sym` [batch], one id per board;
 * sym == NULL makes them those entries, ids without tables fail.  The probabilities come back in the caller's move order,
 * kz_engine_wait_decoded waits for the submit.  An id >= n_sym, or a listed move whose policy_map entry is -1, fails the call
 * that returns the batch, like a move index outside the policy (no read leaves the tables). */
int kz_engine_set_symmetries(kz_engine *engine, int n_sym, const int32_t *square_src, const int32_t *policy_map);
int kz_engine_eval_packed_decoded_sym(kz_engine *engine, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                                      int batch, const uint8_t *sym, const int64_t *move_offsets,
                                      const int32_t *move_indices, float *values_out, float *probs_out);
int kz_engine_submit_packed_decoded_sym(kz_engine *engine, int slot, const uint8_t *bits, size_t bits_stride,
                                        const float *scalars_in, int batch, const uint8_t *sym,
                                        const int64_t *move_offsets, const int32_t *move_indices);

/* ---- every board under every symmetry, averaged: `AverageSymmetryNetwork` (symmetry.rs:70-124,150-184) inside the engine.
 * The caller passes the ORIGINAL boards and the move_to_index lists of the ORIGINAL boards' moves, ONCE per board; outputs
 * have the shape of the other decoded entries (values [batch,5], probabilities parallel to move_indices), and
 * kz_engine_wait_decoded waits for the submit.  The entries use ALL rows of the tables set by kz_engine_set_symmetries, in id
 * order 0 .. n_sym-1: the ROW ORDER OF THE TABLES IS THE SUMMATION ORDER.  The network runs on batch * n_sym virtual boards —
 * virtual board b * n_sym + k is board b under symmetry k, the reference's flat_map order (:98-101) — so batch may be at
 * most max_batch / n_sym.  Per batch three launches on the slot's stream: a fan-out from the pinned staging into device
 * scratch (boards, scalars and move lists replicated, ids = k), the network with its decode exactly as for the _sym entries,
 * and the average into the pinned staging; only batch boards go in and batch results come out over PCIe.
 * Arithmetic, all f32, every division correctly rounded; with v_k, p_k the decoded values and probabilities under symmetry k
 * as the _sym entry produces them and n = n_sym (symmetry.rs:156-176):
 *   each of the five values = (((0 + v_0) + v_1) + ... + v_{n-1}) / n
 *   each probability        = ((0 + p_0 / n) + p_1 / n) + ... + p_{n-1} / n     in the caller's move order
 * and a finished board (an empty range) gets no probabilities.
 * Fails before anything is enqueued, with a message of its own each: no tables set; batch > max_batch / n_sym (the message
 * names that limit); a bad slot; a slot still in flight; null arguments or bad offsets as for the other decoded submits.
 * batch == 0 is the same no-op.  Errors inside the batch — a listed move without an image under some symmetry, a move index
 * outside the policy, a softmax sum that is not positive, a non-finite activation, on ANY virtual board — fail the call that
 * returns the batch with the _sym entries' messages; no read leaves the tables.  kz_engine_set_symmetries refuses while an
 * averaged batch is in flight. */
int kz_engine_eval_packed_decoded_avg(kz_engine *engine, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                                      int batch, const int64_t *move_offsets, const int32_t *move_indices,
                                      float *values_out, float *probs_out);
int kz_engine_submit_packed_decoded_avg(kz_engine *engine, int slot, const uint8_t *bits, size_t bits_stride,
                                        const float *scalars_in, int batch, const int64_t *move_offsets,
                                        const int32_t *move_indices);

/* ---- per-board status and the exact-f32 range fallback ----
 * Every error a launch detects is detected for ONE board (boards are independent columns of every product here), and beside
 * the per-batch verdict of the entries above the engine keeps a status per board, a set of bits: */
#define KZ_BOARD_OK 0
#define KZ_BOARD_BAD_DECODE 1 /* softmax sum not strictly positive, move index outside the policy, id >= n_sym, no image under the symmetry */
#define KZ_BOARD_NONFINITE 2  /* the range check fired for this board */
#define KZ_BOARD_FELL_BACK 4  /* re-evaluated by the range fallback; its results are the exact-f32 ones */
/* A board out of range normally has a NaN softmax sum as well, so it usually carries KZ_BOARD_BAD_DECODE | KZ_BOARD_NONFINITE.
 * kz_engine_wait_decoded_status is kz_engine_wait_decoded, except that an error inside the batch does not fail the call: it
 * returns 0 and *status_out points at uint8_t [batch], library-owned, with the lifetime of the two views (typed void for the
 * bindings' sake).  It serves the plain, _sym and _avg decoded submits; for an averaged batch a board's status is the OR over
 * its n_sym virtual boards.  Boards with status 0 hold exactly what kz_engine_wait_decoded would have given them; the values and
 * probabilities of a board with any other status than exactly KZ_BOARD_FELL_BACK are unspecified, but only that board's own
 * ranges are touched.  Argument, slot and in-flight errors fail as before.
 * kz_engine_eval_packed_decoded_status is kz_engine_eval_packed_decoded_sym (sym == NULL: no symmetry ids) with a caller-owned
 * status_out, uint8_t [batch]. */
int kz_engine_wait_decoded_status(kz_engine *engine, int slot, const float **values_out, const float **probs_out,
                                  void **status_out);
int kz_engine_eval_packed_decoded_status(kz_engine *engine, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                                         int batch, const uint8_t *sym, const int64_t *move_offsets,
                                         const int32_t *move_indices, float *values_out, float *probs_out, void *status_out);
/* The range fallback: dtype = KZ_DTYPE_F32 turns it on, -1 off (the default).  Fails, with a message of its own each, on an
 * engine whose own dtype is KZ_DTYPE_F32, while a batch is in flight, and for any other dtype value.  Turning it on creates —
 * here, so that a failure surfaces here — a sibling engine of the same model on the same device in exact f32 with a small
 * max_batch of its own (at most 64); it shares nothing with this engine's streams and staging (only the cached device weights
 * of other exact-f32 engines of the model).  kz_engine_set_symmetries on the engine reaches the sibling too.
 * With the fallback on, every host-boundary call that returns a batch — kz_engine_wait, kz_engine_wait_view,
 * kz_engine_eval_packed, the decoded waits and evals in their plain, _sym and _avg forms, and the two status entries — looks
 * at the per-board status once the batch is complete and re-evaluates exactly the boards that carry KZ_BOARD_NONFINITE, from
 * the slot's input staging, through the sibling's matching entry (the same symmetry id for _sym, the averaged entry for _avg;
 * averaged batches only while n_sym <= the sibling's max_batch), in chunks, inside the returning call; the sibling's results
 * replace those boards' rows and ranges.  A board whose exact-f32 evaluation is clean gets status KZ_BOARD_FELL_BACK alone,
 * and the calls without a status output then succeed; a board still bad in f32 keeps its bits beside KZ_BOARD_FELL_BACK and
 * those calls fail with the messages they have without the fallback.  KZ_BOARD_BAD_DECODE without KZ_BOARD_NONFINITE is never
 * re-evaluated: that is the caller's move list.  A fell-back board costs a synchronous exact-f32 launch on the calling thread
 * (DESIGN.md 6.4.3).  The device-resident entry points below are outside the fallback and keep failing at
 * kz_engine_synchronize. */
int kz_engine_set_range_fallback(kz_engine *engine, int dtype);

/* ---- shadow audit: a sample of the decoded batches, evaluated a second time in a <= 1e-4 arithmetic ----
 * Answers "is this network, on the positions it is actually asked about, inside the f16 contract?" without a second engine in
 * the caller.  kz_engine_set_audit(engine, dtype, period, boards): dtype = KZ_DTYPE_F32 or KZ_DTYPE_F32_SPLIT16 turns the audit
 * on, -1 off (the default; period and boards are then ignored).  Turning it on creates - here, so that a failure surfaces here -
 * a sibling engine of the same model on the same device in `dtype` with max_batch = min(64, the engine's), hands it the
 * symmetry tables already set (kz_engine_set_symmetries reaches it afterwards) and zeroes the statistics; calling it again
 * while on replaces the settings and zeroes them again.  It is not the range fallback's sibling: both may be on at once.
 * (A KZ_DTYPE_BF16 engine takes either sibling.)
 * Fails, with a message of its own each: dtype equal to the engine's own; KZ_DTYPE_F16 or any other value; KZ_DTYPE_F32_SPLIT16
 * on a model for which kz_model_supports_dtype is 0; period < 1; boards < 1 or larger than the sibling's max_batch; a batch in
 * flight on any slot.
 * The engine counts the decoded submits with batch > 0 - plain, _sym and _avg, and the kz_engine_eval_* forms that go through
 * them - from this call on; submits number 1, 1 + period, 1 + 2 * period ... are audited.  Of an audited batch the FIRST k
 * boards are: k = min(boards, batch), for an averaged batch min(boards, batch, sibling max_batch / n_sym) (0: the batch is not
 * audited and counts nowhere).  Right after the batch's own launch is enqueued those k boards go, from the slot's pinned input
 * staging, to the sibling's slot of the same index through the matching entry (the same symmetry ids, or the averaged entry),
 * and run there on the sibling's own stream beside the batch; a failing sibling submit fails the submit with its message (the
 * slot is then free).  The call that returns the batch - after the per-board status and after the range fallback - waits for
 * the sibling and compares on the host.  No result, status or verdict of any batch changes.  kz_engine_submit_packed,
 * kz_engine_eval_dense and the device-resident entry points are outside the audit.
 * A sampled board is compared only when its status is exactly KZ_BOARD_OK on both sides (after the fallback); every other one,
 * a fell-back board included, adds 1 to `skipped`.  Per compared board, in batch order, for each of its five values and then
 * for each of its probabilities in the caller's move order: d = fabsf(engine - sibling) in f32, max = fmaxf(max, d),
 * sum_sq += (double)d * (double)d, accumulated sequentially; batches accumulate in the order they are returned.
 * kz_engine_audit_stats copies the totals and, with reset != 0, zeroes them afterwards; it fails while the audit is off and
 * while an audited batch is still in flight; `out` is a kz_audit_stats * (typed void for the bindings' sake, like the status
 * outputs above).  With the audit off a decoded submit and a returning call pay one pointer test. */
typedef struct kz_audit_stats {
    int64_t batches;          /* audited batches that were returned */
    int64_t boards;           /* boards compared */
    int64_t moves;            /* probabilities compared */
    int64_t skipped;          /* sampled boards left out: status != KZ_BOARD_OK on either side */
    float   max_abs_value[5]; /* per decoded column: value, win, draw, loss, moves_left */
    float   max_abs_prob;
    double  sum_sq_value[5];
    double  sum_sq_prob;
} kz_audit_stats;
int kz_engine_set_audit(kz_engine *engine, int dtype, int period, int boards);
int kz_engine_audit_stats(kz_engine *engine, void *out, int reset);

/* ---- stream shift and range profile: f16 for a network whose residual stream leaves +-65504 ----
 * A ResTower is positively homogeneous in its residual stream: with s = 2^-k, the stem's weights and bias and every block
 * convolution's folded bias times s, and the final BatchNorm's scale divided by s, give the SAME function with a stream s times
 * as large — exactly, s being a power of two.  f16 holds 30 binades: a stream that reaches 1e6 fits after a shift.
 * kz_model_stream_shift(model, k, &out) returns a new immutable model — an ordinary kz_model, to be freed with kz_model_free,
 * independent of `model` — whose folded tensors are the source's except: the stem convolution's weights and bias times 2^-k,
 * the folded bias of each of the 2 * depth block convolutions times 2^-k, the final BatchNorm's scale times 2^k.  Block weights,
 * the final BatchNorm's shift, the heads and the descriptor (kz_model_get_info, kz_model_plan for every dtype and max_batch)
 * are bit-identical.  k in [-24, 24]; a negative k ENLARGES the stream; k = 0 copies.  Fails, with a message of its own each:
 * an AttentionTower network (LayerNorm re-normalises: there is nothing to shift), a DenseNetwork, a tower without blocks, k out
 * of range, and a non-zero value that would leave f32's normal range (nothing is rounded silently).
 * Every entry point works on the result unchanged; engines of it have device weights of their own.  What the shift moves
 * is every tensor in front of the final BatchNorm: kz_engine_read_activation on a shifted model returns the SHIFTED stream
 * ("tower.0" .. "tower.<d>" and the ".mid" ones times 2^-k; "tower.<d+1>" / "tower.out" as before).
 * What it costs below: a stored value under 2^-14 becomes an f16 subnormal, absolute error at most 2^-25 in the shifted
 * stream = 2^(k-25) in the unshifted stream's units (in-range values keep their 11 bits: the relative error does not change).
 * What it cannot reach: the output of the final BatchNorm and the heads' hidden layers — they are the same tensors as before.
 *
 * The range profile measures what k has to be: max |x| of every tensor an f16 or split16 kernel of the tower stores, on the
 * caller's positions, on the GPU in exact f32.  The sites, 2 * tower_depth + 1 of them, in this order and with the names
 * of kz_engine_read_activation: "tower.0" (the stem's output), then per block i = 1 .. d "tower.<i>.mid" and "tower.<i>" —
 * except that the last block's output exists only behind the final BatchNorm: the last site is "tower.<d+1>", and it is the
 * ONLY site a shift does not move.  kz_model_range_sites / kz_model_range_site_name (buf of at least 24 bytes) tell; both,
 * and the profile, fail for a network without a ResTower or without blocks.
 * kz_model_range_profile is synchronous: it creates an internal exact-f32 engine of the model on `device` on the per-layer
 * path ("conv_igemm_f32", whatever kz_model_plan says; no environment switch is read) with max_batch = min(batch, 64),
 * evaluates the tower on the boards (packed as for kz_engine_eval_packed) in chunks, and destroys the engine.
 * site_max_out [n_sites]: max |x| over all boards; board_max_out [batch] (may be NULL): per board, the max over the sites a shift
 * moves (all but the last).  A non-finite value (inf or NaN) reports +inf, never NaN, and a board reports +inf from its first
 * non-finite site on (behind one the values are not the network's: ReLU turns a NaN into 0); other boards are not affected.
 * The values are maxima of exact-f32 tensors: the same for any batch split and any scheduling.
 * Choosing k: with m the maximum over the shifted sites (all but the last; = max of board_max_out),
 *     k = max(0, ceil(log2(m / 65504)) + headroom_bits)
 * The library reports and applies, the caller decides; the bindings implement the rule (capi.shift_for, HipNetwork::shift_for,
 * hip.rs shift_for) and the tools default to 2 bits of headroom: positions not yet seen can be larger than the profiled ones.
 *
 * kz_model_range_profile_fast is the same call — the same sites and names, site_max_out and board_max_out, the same non-finite
 * rule and refusals — at the rate of the one-launch exact-f32 tower: where that kernel takes the network (128 / 256 tower
 * channels on a small board: "tower_resident_f32" of kz_model_plan, with or without "+heads") the internal engine runs ONE launch
 * per chunk, whose epilogues take the maxima of what they store while the tensors are in LDS; no head kernel, no decode and no
 * copy of the tower output runs, max_batch = min(batch, 256), and the device weight stream is the one ordinary exact-f32 engines
 * of the model share.  Every other network (Go 19x19, other widths) runs exactly kz_model_range_profile.  On exactly
 * representable tensors the two entries return the same bits; otherwise they differ as two exact-f32 summation orders do
 * (1e-4 relative).  kz_model_range_profile_fast_path writes which of the two it is, "tower_resident_f32" or "conv_igemm_f32"
 * (buf of at least 24 bytes), without touching a GPU; it fails where the profile fails. */
int kz_model_stream_shift(const kz_model *model, int k, kz_model **out);

/* ---- int8 calibration: what KZ_DTYPE_INT8 needs of a model ----
 * kz_model_quantize_int8(model, site_max, n_sites, &out) returns a new immutable model, independent of `model` and freed with
 * kz_model_free, whose f32 tensors and descriptor are the source's bit for bit — every other dtype's engines of it return what
 * they return on the source — with a calibration beside them: site_max [n_sites] is max |x| of every range site on the caller's
 * positions (kz_model_range_profile_fast's site_max_out, times any headroom), in the sites' order.  No GPU is touched, and the
 * calibration lives in memory only: the .kzm container does not change.  The arithmetic of an engine of dtype 4 on the result,
 * every scale a power of two (exact to apply), the roundings exactly these:
 *   activation exponent of site s:  e_s = ceil(log2(site_max[s] / 127)); a quantised image holds
 *     q = clamp(rne(v * 2^-e_s), -127, 127) as int8, rne to nearest even; -128 is never produced
 *   weight exponent per (block convolution, output channel), on the folded Conv+BN weights:
 *     f = ceil(log2(max |w[oc,:,:,:]| / 127)), wq = rne(w * 2^-f); an all-zero filter has f = 0
 *   a block convolution, per output element: acc = the i32 sum of wq * q over 9 taps x C (exact); t = (float)acc (nearest even);
 *     v = t * 2^(e_in + f_oc) + bias[oc] (one rounding); ReLU
 *   conv A stores quant(v, e_mid).  Conv B adds the f16 stream x to v in f32, after the ReLU, then stores x = f16(v) and
 *     quant(v, e_next), both from the same f32 v.  The stem is the f16 engine's and stores f16(v) and quant(v, e_0).  The last
 *     layer: ReLU, residual add, final BN in f32, f16 rows out — the last range site is not quantised, and its site_max entry
 *     is accepted and ignored.
 * Fails, with a message of its own each: a null argument, n_sites != kz_model_range_sites, an entry among the first n_sites - 1
 * that is not finite or not > 0 (or whose exponent is beyond +-64), an AttentionTower network, a DenseNetwork, a tower without
 * blocks, a model that is calibrated already.  kz_model_stream_shift refuses a calibrated model: shift first, then calibrate.
 * kz_model_int8_site_exponents writes e_s of the n_sites - 1 quantised sites; it fails on a model that is not calibrated. */
int kz_model_quantize_int8(const kz_model *model, const float *site_max, int n_sites, kz_model **out);
int kz_model_int8_site_exponents(const kz_model *model, int *exp_out /* [n_sites - 1], 32-bit */);

int kz_model_range_sites(const kz_model *model, int *n_sites);
int kz_model_range_site_name(const kz_model *model, int site, char *buf, size_t len);
int kz_model_range_profile(const kz_model *model, int device, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                           int batch, float *site_max_out, float *board_max_out);
int kz_model_range_profile_fast(const kz_model *model, int device, const uint8_t *bits, size_t bits_stride,
                                const float *scalars_in, int batch, float *site_max_out, float *board_max_out);
int kz_model_range_profile_fast_path(const kz_model *model, char *buf, size_t len);

/* ---- range histogram: how much of every stored tower tensor sits in each binade ----
 * The profile above measures one end of the distribution, max |x|.  The histogram counts every stored value of every site by
 * binade, exactly, so that for any shift k and any arithmetic the caller can read off the share of stored values that overflow
 * f16, become f16 subnormals, flush to zero, or lose the lo half of a split16 pair (the bindings' shift_report does the sums).
 * The bins, KZ_RANGE_BINS of them.  For a stored f32 value with bit pattern u, let a = u & 0x7fffffff and e = a >> 23:
 *   a == 0 (+-0)             bin 0
 *   e == 255 (inf or NaN)    bin 95
 *   otherwise                E = e - 127 (an f32 subnormal counts as E = -127); bin = clamp(E, -50, 43) + 51:
 *                            bin b in 2 .. 93 holds 2^(b-51) <= |x| < 2^(b-50), bin 1 holds 0 < |x| < 2^-49, bin 94 holds
 *                            finite |x| >= 2^43
 * This resolves f16's whole window under every k in [-24, 24]: the smallest subnormal half, 2^-25, at k = -24 is bin 2, and
 * 2^16 at k = 24 is bin 91.  The binning is integer arithmetic on the bit pattern, never a floating comparison.
 * kz_model_range_histogram has kz_model_range_profile's contract — the same sites in the same order, the same refusals (each
 * in this function's name), the same internal exact-f32 per-layer engine and chunks — and fills hist_out [n_sites][KZ_RANGE_BINS]:
 * the number of elements of each site's tensors, over all boards and over real channels only, per bin.  Every element is
 * counted once: a site's 96 counts sum to batch * h * w * tower_channels.  What is counted is the value that is stored (after
 * ReLU, the residual add and the final BatchNorm), as for the maxima.  The counts are integers: they do not depend on the batch
 * split, a board's place, or scheduling.  A non-finite value lands in bin 95; what the later sites hold for THAT board is
 * unspecified (ReLU turns a NaN into 0), its elements are still counted once per site, and no other board's counts change.
 * kz_model_range_histogram_fast is the same call inside the one-launch exact-f32 tower wherever
 * kz_model_range_profile_fast_path says "tower_resident_f32" (the epilogues bin what they store while it is in LDS; the device
 * weight stream is the one ordinary exact-f32 engines of the model share), and exactly kz_model_range_histogram elsewhere.  On
 * exactly representable tensors the two return the same counts; otherwise they differ where two exact-f32 summation orders
 * put a value on different sides of a binade boundary.  (hist_out: uint64_t [n_sites][KZ_RANGE_BINS], typed void like the
 * status bytes of kz_engine_wait_status.) */
#define KZ_RANGE_BINS 96
int kz_model_range_histogram(const kz_model *model, int device, const uint8_t *bits, size_t bits_stride, const float *scalars_in,
                             int batch, void *hist_out);
int kz_model_range_histogram_fast(const kz_model *model, int device, const uint8_t *bits, size_t bits_stride,
                                  const float *scalars_in, int batch, void *hist_out);

/* ---- tower taps and error profile: what the one-launch towers store, and how far it is from exact f32 ----
 * The profile and the histogram above run in exact f32: they say what a 16-bit store WOULD do.  A tap is what the kernel that
 * ships DID store.  Every one-launch ResTower ("tower_resident_f16", "_f16g", "_bf16g", "_split16", "_f32" of kz_model_plan) has
 * a tap instance per geometry: the same template arguments, the same arithmetic in the same order, and one more store — the lane
 * that writes its four channels of a pixel to the LDS image writes the same elements, as rounded for that store (f16, bf16, the
 * (hi, lo) pair, f32), to a tensor in device memory, at every range site (kz_model_range_site_name's sites and order).  The last
 * site is what the plain tower hands on: f32 where its output tensor is f32 (split16, bf16, f32), f16 in the two f16 launches.
 * Only rows of real boards are written — not the rows that fill a 16-row tile, a missing partner board, or tiles past `batch`.
 * A tap instance is the plain tower: no heads, no decode.
 *
 * kz_model_tower_taps_path(model, max_batch, dtype, buf, len) writes the kernel a tap call runs — kz_model_plan(model, max_batch,
 * dtype)'s tower_path without "+heads" — without touching a GPU (buf of at least 32 bytes).  max_batch chooses the instance as it
 * does for an engine (boards per workgroup, wide tiles), and the environment switches act as they do for kz_engine_create; a tap
 * call runs THAT geometry on however few boards it is given.
 * kz_model_tower_taps is synchronous: an internal engine of the model on `device`, the boards (packed as for
 * kz_engine_eval_packed) in chunks, every device tensor below 2 GiB.  out: f32 [n_sites][batch][tower_channels][h][w] for the
 * sites [site_first, site_first + n_sites); an element is the stored value widened exactly, (float)hi + (float)lo for a pair.
 * A stream-shifted model's taps are in shifted units.
 * kz_model_error_profile fills out [kz_model_range_sites] of kz_site_error (typed void like hist_out): dtype's taps against exact
 * f32 on the same boards, reduced on the device.  a = the tap, r = the reference; an element where either is not finite counts
 * in `nonfinite` and in no other field.  The reference is the one-launch f32 tower's own taps where kz_model_range_profile_fast_path
 * says "tower_resident_f32", and kz_model_range_profile's per-layer exact-f32 engine at its sites elsewhere.  max_abs_err, max_abs_ref,
 * count and nonfinite do not depend on scheduling; the two sums are f64 and depend on the order of addition in their last bits.
 * dtype: KZ_DTYPE_F16, KZ_DTYPE_F32_SPLIT16 or bf16 (3); KZ_DTYPE_F32 is refused (a profile against itself compares nothing).
 * All three fail, each with a message of its own in the function's name: null arguments; an AttentionTower network; a
 * DenseNetwork; a tower without blocks; a dtype the model does not support; a network whose plan at (max_batch, dtype) runs per
 * layer (read those with KZ_KEEP_ACTIVATIONS and kz_engine_read_activation); a site range outside 0 .. n_sites; batch < 1 or
 * batch > max_batch; a bits_stride below kz_model_info.bits_bytes.  Those checks need no GPU. */
typedef struct kz_site_error {
    double   max_abs_err; /* max |a - r|, the difference taken in f64 */
    double   sum_sq_err;  /* sum (a - r)^2 */
    double   sum_sq_ref;  /* sum r^2 */
    double   max_abs_ref; /* max |r| */
    uint64_t count;       /* elements compared: batch * tower_channels * h * w less nonfinite */
    uint64_t nonfinite;   /* elements where a or r is inf or NaN */
} kz_site_error; /* 48 bytes */
int kz_model_tower_taps_path(const kz_model *model, int max_batch, int dtype, char *buf, size_t len);
int kz_model_tower_taps(const kz_model *model, int device, int max_batch, int dtype, const uint8_t *bits, size_t bits_stride,
                        const float *scalars_in, int batch, int site_first, int n_sites, float *out);
int kz_model_error_profile(const kz_model *model, int device, int max_batch, int dtype, const uint8_t *bits, size_t bits_stride,
                           const float *scalars_in, int batch, void *out);

/* ---- int8 taps and error profile: every stored int8 image, its error and its clamp count ----
 * The three entries above refuse the int8 dtypes (4, 5, 8): an int8 tower stores int8 images at a scale per site, which their
 * element formats do not hold.  These three are the int8 towers' own, for a CALIBRATED ResTower model.  The range sites are
 * kz_model_range_sites': 2 * depth + 1, in kz_model_range_site_name's order.  Site 0 (the stem) and every block output but the
 * last store an image X8 = quant(v, e_s) and, beside it from the same f32 v, the residual-stream value X = f16(v); a mid site
 * stores an image Y8 only; the last site stores the f16 tower output behind the final BN and no image (kz_model_quantize_int8
 * states the arithmetic).  A tap is what the launch DID store: the one-launch tower ("tower_resident_i8") has a tap instance per
 * geometry of the tower alone — the same arithmetic in the same order and, behind each epilogue store, the same q bytes and f16
 * values once more to device memory, rows of real boards only —; the per-layer plan ("board_conv_i8") keeps its images in
 * device memory already, and a tap engine copies every layer's outputs behind that layer's launch.
 *
 * kz_model_int8_taps_path(model, max_batch, dtype, buf, len) writes the kernel a tap call runs, "tower_resident_i8" or
 * "board_conv_i8", never with "+heads", without touching a GPU (buf of at least 32 bytes).  dtype 5 taps what dtype 4 taps: the
 * tower's bits are dtype 4's, and a tap engine never carries heads, so its wide levels are the tower's own.  dtype 8 taps that
 * tower wherever dtype 5 has a plan, and the per-layer kernel elsewhere.  The one-launch tower chooses its wide level per launch
 * from its batch: a tap call runs the level an engine of max_batch runs at `batch` boards (kz_model_launch_geometry(model,
 * max_batch, 4, batch)), "the batch size whose geometry is tapped".
 * kz_model_int8_taps is synchronous, in chunks, every device tensor below 2 GiB.  image_out (int8_t elements, typed void like
 * hist_out): int8 [n_sites][batch][C][h][w] with
 * C the model's own tower channels (channels the kernels widen the tower by are not returned): the q the epilogue stored; the
 * last site has no image and returns 0.  stream_out: f32 of the same shape: the f16 value stored beside the image, widened; at
 * the last site the f16 tower output; a mid site has no stream and returns NaN.  Either pointer may be NULL, not both.  The
 * image part of the tap buffer is filled with 0x80 before every pass — the contract never produces -128 —, the stream part with
 * NaN patterns: an element no lane wrote comes back as -128, or NaN.
 * kz_model_int8_error_profile fills out [kz_model_range_sites] of kz_int8_site_error (typed void like hist_out), reduced on the
 * device against exact f32 on the same boards — kz_model_error_profile's references: the one-launch f32 tower's own taps where
 * kz_model_range_profile_fast_path says "tower_resident_f32", the per-layer exact-f32 engine elsewhere.  The six fields of each
 * kz_site_error are defined as above; an image element of -128 counts in image.nonfinite.  at_clamp counts what the launch
 * stored at the clamp, an upper bound on what it clamped; ref_beyond counts what an ideal int8 image of the exact network would
 * clamp (127.5 is the contract's own tie: rne(127.5) = 128).  Both run over real channels of real boards only.
 * All three fail, each with a message of its own in the function's name, in front of any GPU call: null arguments; a dtype that is
 * not an int8 dtype; an AttentionTower network; a DenseNetwork; a tower without blocks; a model that is not calibrated; a shape
 * the dtype refuses (kz_model_plan's reason); a site range outside 0 .. n_sites; batch < 1 or batch > max_batch; a bits_stride
 * below kz_model_info.bits_bytes. */
typedef struct kz_int8_site_error {
    kz_site_error image;  /* a = q * 2^e_s (exact in f32) against r; count 0 at the last site */
    kz_site_error stream; /* a = the f16 stream value against r; count 0 at a mid site */
    uint64_t at_clamp;    /* image elements with |q| == 127 */
    uint64_t ref_beyond;  /* elements whose reference is finite and has |r| * 2^-e_s >= 127.5 */
    int32_t  exponent;    /* e_s; 0 at the last site */
    int32_t  reserved;    /* 0 */
} kz_int8_site_error; /* 120 bytes */
int kz_model_int8_taps_path(const kz_model *model, int max_batch, int dtype, char *buf, size_t len);
int kz_model_int8_taps(const kz_model *model, int device, int max_batch, int dtype, const uint8_t *bits, size_t bits_stride,
                       const float *scalars_in, int batch, int site_first, int n_sites, void *image_out, float *stream_out);
int kz_model_int8_error_profile(const kz_model *model, int device, int max_batch, int dtype, const uint8_t *bits, size_t bits_stride,
                                const float *scalars_in, int batch, void *out);

/* ---- device-resident evaluation (inputs and outputs already in HBM; used by bench.py and the parity tests) ----
 * Pointers are device pointers on the engine's device (kz_device_malloc).  Enqueues on the engine's stream and
 * returns; kz_engine_synchronize waits. */
int kz_engine_enqueue_packed_device(kz_engine *engine, const void *d_bits, size_t bits_stride,
                                    const void *d_scalars_in, int batch, void *d_scalars_out, void *d_policy_out);
int kz_engine_enqueue_dense_device(kz_engine *engine, const void *d_input_nchw, int batch, void *d_scalars_out,
                                   void *d_policy_out);
int kz_engine_synchronize(kz_engine *engine);

/* ---- device memory helpers (plain hipMalloc/hipMemcpy on `device`) ---- */
int kz_device_malloc(int device, size_t bytes, void **out);
int kz_device_free(int device, void *ptr);
int kz_memcpy_h2d(int device, void *dst, const void *src, size_t bytes);
int kz_memcpy_d2h(int device, void *dst, const void *src, size_t bytes);
int kz_device_synchronize(int device);

/* ---- measurement ----
 * With profiling on, every kernel launch of the forward pass is bracketed by HIP events on the engine's stream.
 * kz_engine_kernel_time sums the elapsed time of the launches whose kernel name starts with `prefix` since
 * profiling was last enabled (it synchronizes the stream first). */
int kz_engine_set_profiling(kz_engine *engine, int enable);
int kz_engine_kernel_time(kz_engine *engine, const char *prefix, double *total_ms, int64_t *launches);
/* Environment switches read by kz_engine_create.  This is the COMPLETE list for libkzhip.so (tests/test_abi.py compares
 * it with the strings in the built library); each selects between product paths that are parity-tested against the
 * oracle, none changes results beyond summation order, all are off by default:
 *   KZ_FORCE_GENERIC=1      no one-launch tower: one launch per layer ("board_conv_f16" / "conv_igemm_*"); an AttentionTower
 *                           network: the vector-ALU kernel ("attention_tower_f32_valu") instead of the matrix-core launch
 *   KZ_NO_BOARD_CONV=1      per-layer f16 convolutions through the implicit-GEMM kernel instead of the board-tile kernel
 *   KZ_NO_RESIDENT_F16G=1   no "tower_resident_f16g" launch (f16 shapes other than the chess network go per layer)
 *   KZ_NO_FUSED_HEADS=1     the "...+heads" launches without their heads: tower launch + separate head kernels
 *   KZ_TOWER_NB=1|2         boards per workgroup of the chess f16 launch (default 2; 1 = twice the workgroups: the better
 *                           choice for ONE engine at batch <= 256)
 *   KZ_KEEP_ACTIVATIONS=1   with KZ_FORCE_GENERIC=1: keep every layer's output for kz_engine_read_activation
 * The kernel organisations that were measured and rejected (four boards per workgroup, two Go boards per workgroup,
 * 32x32x16 tiles, hipGraph replay, ablation knobs) are NOT in this library nor in its source directory: `experiments/build.sh`
 * builds them (experiments/csrc/) into a separate experiments/libkzhip_exp.so for tests/test_gpu_experiments.py.
 *
 * Name of the path the engine chose; DESIGN.md 5.0 has the table (shape x arithmetic -> path, launches per batch, measured
 * rate), printed from kz_model_plan by tools/gen_path_table.py and held to the built library by tests/test_path_table.py.
 * One launch for the whole tower: "tower_resident_f16+heads" (chess attention
 * network — ChessStdMapper or ChessHistoryMapper input planes —, heads included), "tower_resident_f16",
 * "tower_resident_f16g" (other board-resident f16 shapes: 64 .. 512 channels on small boards),
 * "tower_resident_f16g+heads" (the same with the conv policy head and the scalar head inside: 128 / 256 channels),
 * "tower_resident_f32+heads" (exact f32, conv policy heads: decode, tower and heads in one launch), "tower_resident_f32"
 * (exact f32, other heads), "tower_resident_split16+heads" (KZ_DTYPE_F32_SPLIT16: the chess attention network at 256
 * channels and the conv-policy networks at 128 / 256 channels: encode, tower, scalar head and policy head in one launch),
 * "tower_resident_split16" (the other shapes of
 * KZ_DTYPE_F32_SPLIT16: tower launch + f32 head kernels), "tower_resident_bf16g+heads" / "tower_resident_bf16g"
 * (KZ_DTYPE_BF16: conv policy heads at 128 / 256 channels inside; else tower launch + f32 head kernels), "tower_resident_i8"
 * (KZ_DTYPE_INT8, and KZ_DTYPE_INT8_HEADS elsewhere: tower launch + f16 head kernels) / "tower_resident_i8+heads"
 * (KZ_DTYPE_INT8_HEADS: conv policy heads, scalar head and decode inside).  One launch per layer:
 * "board_conv_f16" (whole boards as LDS tiles, Go-size boards), "board_conv_split16" (the same per-layer kernel in split
 * arithmetic: KZ_DTYPE_F32_SPLIT16 on boards the one-launch split tower cannot hold), "conv_igemm_f16", "conv_igemm_f32".
 * Networks whose tower is the reference's AttentionTower (python/lib/model/attention.py:8-45) instead of the ResTower — one
 * launch for the tower: "attention_tower_f16" / "attention_tower_f32" (8x8 boards, 8 heads of d_k = d_v = 16, d_model 128 / 256:
 * f16 and exact f32 on the matrix cores), "attention_tower_f32_valu" (every other shape: exact f32 on the vector ALUs; an f16
 * engine reads and writes f16 rows around it).  KZ_DTYPE_F32_SPLIT16 and KZ_DTYPE_BF16 have no AttentionTower kernel: kz_model_supports_dtype = 0.
 * "dense_network_f32": a DenseNetwork (python/lib/model/simple.py), the whole network in one launch, f32 arithmetic. */
const char *kz_engine_tower_path(const kz_engine *engine);
/* How the dominant launch of that path covers the chip for a batch of `batch` boards: workgroups per launch and boards
 * per workgroup (per-layer paths: boards_per_workgroup = 0 when a workgroup holds a tile, not whole boards). */
int kz_engine_launch_geometry(const kz_engine *engine, int batch, int *workgroups, int *boards_per_workgroup);
/* The same answer without an engine: what an engine of (max_batch, dtype) on this model reports for `batch` (0 <= batch <=
 * max_batch).  Host logic like kz_model_plan — no GPU is touched — with kz_model_plan's refusals under this function's name. */
int kz_model_launch_geometry(const kz_model *model, int max_batch, int dtype, int batch, int *workgroups, int *boards_per_workgroup);

/* ---- debugging / parity: copy an intermediate activation of the last evaluation to the host as f32 NCHW.
 * name: "tower.<i>" as in python/lib/model/post_act.py's nn.Sequential indices (0 = stem, 1..d = blocks,
 * d+1 = final BN): only available when the engine was created with the generic per-layer path (set KZ_FORCE_GENERIC=1
 * and KZ_KEEP_ACTIVATIONS=1 in the environment before kz_engine_create); or "tower.out", the tower's output (after the
 * final BN), on every path that writes it to memory (all but the "...+heads" paths; KZ_NO_FUSED_HEADS=1 in the
 * environment before kz_engine_create gives the separate head launches back).
 * On a model made by kz_model_stream_shift the activations in front of the final BN are the SHIFTED stream's (2^-k times the
 * source model's); "tower.<d+1>" and "tower.out" are the source's. */
int kz_engine_read_activation(kz_engine *engine, const char *name, int batch, float *out_nchw);

#ifdef __cplusplus
}
#endif
#endif /* KZ_HIP_H */
