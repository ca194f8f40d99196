//! kz-core/src/network/hip.rs — `HipNetwork`: the MI355X executor behind kZero's `Network` trait.
//!
//! Drop-in sibling of `CudaNetwork` (kz-core/src/network/cudnn.rs:18-88): same constructor shape, same
//! `Network<B>` contract (kz-core/src/network/mod.rs:52-63), same `decode_output` (network/common.rs:16-100).
//! The arithmetic lives in libkzhip.so (C ABI: include/kz_hip.h); this file only binds it.
//!
//! Differences from `CudaNetwork`, all invisible to callers:
//!  * the mapper's *packed* output (`InputMapper::encode_input`: BitBuffer + scalars, mapping/mod.rs:37) is handed
//!    over as is; the dense f32 expansion (`encode_input_full`, mapping/mod.rs:40-63) happens on the GPU;
//!  * no NaN padding (cudnn.rs:65) up to `max_batch_size` and no input clone (cudnn.rs:70): only `batch` rows exist;
//!  * `decode_output`'s gather + softmax (common.rs:60-86) runs on the GPU by default (`KZ_HIP_DECODE=device`): the
//!    executor thread builds the `move_to_index` list of every board when it submits the batch, the GPU returns
//!    tanh(value), softmax(wdl) and the per-move probabilities — 0.2 KB instead of 7.5 KB per chess evaluation over
//!    PCIe and no softmax on this thread.  Measured with the C++ mirror of this file (tests/cpp/bench_executor.cpp,
//!    chess 20x256 f16, ONE executor thread, move generation + a SipHash lookup per move on it): host decode
//!    257-350k evals/s box to box (the thread is the bottleneck: 3.2-3.9 CPU-s per million evaluations), device decode
//!    404-505k with the thread working 0.8-0.9 of a core, the GPU alone 482-527k.  `KZ_HIP_DECODE=host` keeps the reference's own `decode_output` call (bit-identical softmax; set
//!    gpu_threads_per_device >= 4 with it for a 256-channel chess network in f16).  Since round 5 the gather + softmax is
//!    the last step of the network's own launch (one launch per batch, no copy operations: 532k) and
//!  * a batch's host work before the launch (`encode_input` of every board, `move_to_index` of every available move) is
//!    shared with `KZ_HIP_PREP_THREADS` scoped helper threads when asked for (default 0: all of it on the executor
//!    thread, which is what the committed seam figures of the default were measured with on the C++ mirror; the mirror's
//!    helper is a persistent thread, the scoped threads here spawn per batch — a different cost model that has not been
//!    compiled or timed, so it is opt-in): `prepare` below.
//!
//! NOT compiled in this repository's CI (no cargo in the build image); written against the cited signatures.

use std::collections::VecDeque;
use std::borrow::Borrow;
use std::ffi::{c_char, c_int, c_void, CStr, CString};
use std::fmt::{Debug, Formatter};
use std::marker::PhantomData;
use std::sync::{Arc, Mutex, OnceLock};

use board_game::board::Board;
use internal_iterator::InternalIterator;

use crate::mapping::bit_buffer::BitBuffer;
use crate::mapping::BoardMapper;
use crate::network::common::decode_output;
use crate::network::{Network, ZeroEvaluation};
use crate::zero::values::ZeroValuesPov;
use board_game::pov::ScalarPov;
use board_game::wdl::WDL;
use std::borrow::Cow;

#[repr(C)]
#[derive(Debug, Default, Copy, Clone)]
pub struct KzModelInfo {
    pub input_channels: i32,
    pub board_h: i32,
    pub board_w: i32,
    pub input_scalar_channels: i32,
    pub input_bool_channels: i32,
    pub policy_len: i32,
    pub tower_depth: i32,
    pub tower_channels: i32,
    pub policy_kind: i32,
    pub bits_bytes: i32,
    pub param_count: i64,
    pub flops_per_eval: f64,
}

/// What `kz_engine_create` would choose for a model (kz_model_plan): host logic, no GPU touched
#[repr(C)]
#[derive(Debug, Copy, Clone)]
pub struct KzPathPlan {
    pub tower_path: [c_char; 48],
    pub launches_per_batch: i32,
    pub reserved: [i32; 3],
}

/// What the shadow audit has accumulated (`kz_audit_stats`, include/kz_hip.h; 104 bytes)
#[repr(C)]
#[derive(Debug, Default, Copy, Clone)]
pub struct KzAuditStats {
    pub batches: i64,
    pub boards: i64,
    pub moves: i64,
    pub skipped: i64,
    pub max_abs_value: [f32; 5],
    pub max_abs_prob: f32,
    pub sum_sq_value: [f64; 5],
    pub sum_sq_prob: f64,
}

pub const KZ_DTYPE_F32: c_int = 0;
pub const KZ_DTYPE_F16: c_int = 1;
/// f32 tensors and the same <= 1e-4 parity as KZ_DTYPE_F32, the tower's products as three f16 MFMAs on (hi, lo) pairs
pub const KZ_DTYPE_F32_SPLIT16: c_int = 2;
pub const KZ_DTYPE_BF16: i32 = 3;
/// f16 tensors, the tower's block convolutions on the i8 matrix cores: a calibrated model only (`kz_model_quantize_int8`)
pub const KZ_DTYPE_INT8: i32 = 4;
/// dtype 4's tower with the conv policy heads, the scalar head and the decode inside its launch where it can carry them
/// ("tower_resident_i8+heads"); everywhere else exactly dtype 4's plan
pub const KZ_DTYPE_INT8_HEADS: i32 = 5;
pub const KZ_ENGINE_SLOTS: usize = 4;
/// Per-board status bits of `kz_engine_wait_decoded_status` / `kz_engine_eval_packed_decoded_status` (include/kz_hip.h)
pub const KZ_BOARD_OK: u8 = 0;
pub const KZ_BOARD_BAD_DECODE: u8 = 1;
pub const KZ_BOARD_NONFINITE: u8 = 2;
pub const KZ_BOARD_FELL_BACK: u8 = 4;

// The C ABI of include/kz_hip.h, declaration for declaration (tests/test_rust_shim_text.py compares the two files:
// every function of the header is bound here with the same name, arity and pointer-ness).  `kz_model` / `kz_engine`
// are opaque: `*mut c_void` / `*const c_void`.
#[link(name = "kzhip")]
extern "C" {
    fn kz_last_error() -> *const c_char;
    fn kz_device_count(count: *mut c_int) -> c_int;
    fn kz_device_pci_bus_id(device: c_int, buf: *mut c_char, len: usize) -> c_int;
    fn kz_model_load(path: *const c_char, out: *mut *mut c_void) -> c_int;
    fn kz_model_load_memory(blob: *const c_void, len: usize, out: *mut *mut c_void) -> c_int;
    fn kz_model_load_onnx(path: *const c_char, input_scalar_channels: c_int, out: *mut *mut c_void) -> c_int;
    fn kz_model_load_onnx_memory(blob: *const c_void, len: usize, input_scalar_channels: c_int, out: *mut *mut c_void) -> c_int;
    fn kz_model_free(model: *mut c_void);
    fn kz_model_get_info(model: *const c_void, out: *mut KzModelInfo) -> c_int;
    fn kz_engine_create(model: *const c_void, device: c_int, max_batch: c_int, dtype: c_int, out: *mut *mut c_void) -> c_int;
    fn kz_engine_destroy(engine: *mut c_void);
    fn kz_model_supports_dtype(model: *const c_void, dtype: c_int) -> c_int;
    fn kz_model_plan(model: *const c_void, max_batch: c_int, dtype: c_int, out: *mut KzPathPlan) -> c_int;
    fn kz_model_launch_geometry(model: *const c_void, max_batch: c_int, dtype: c_int, batch: c_int, workgroups: *mut c_int, boards_per_workgroup: *mut c_int) -> c_int;
    // stream shift (a new model: the same function, the residual stream 2^-k times as large) and the exact-f32 range profile
    fn kz_model_stream_shift(model: *const c_void, k: c_int, out: *mut *mut c_void) -> c_int;
    // int8 calibration (a new model: the same tensors with an exponent per range site beside them; the only kind dtype 4 takes).
    // No KZ_HIP_DTYPE=int8 yet: the shim has no calibration policy of its own.
    fn kz_model_quantize_int8(model: *const c_void, site_max: *const f32, n_sites: c_int, out: *mut *mut c_void) -> c_int;
    fn kz_model_int8_site_exponents(model: *const c_void, exp_out: *mut c_int) -> c_int;
    fn kz_model_range_sites(model: *const c_void, n_sites: *mut c_int) -> c_int;
    fn kz_model_range_site_name(model: *const c_void, site: c_int, buf: *mut c_char, len: usize) -> c_int;
    fn kz_model_range_profile(model: *const c_void, device: c_int, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, site_max_out: *mut f32, board_max_out: *mut f32) -> c_int;
    // ... the same profile inside the one-launch exact-f32 tower where that kernel takes the network, and which of the two it is
    fn kz_model_range_profile_fast(model: *const c_void, device: c_int, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, site_max_out: *mut f32, board_max_out: *mut f32) -> c_int;
    fn kz_model_range_profile_fast_path(model: *const c_void, buf: *mut c_char, len: usize) -> c_int;
    // the range histogram: binade counts of every stored tower tensor, hist_out u64 [n_sites][KZ_RANGE_BINS]
    fn kz_model_range_histogram(model: *const c_void, device: c_int, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, hist_out: *mut c_void) -> c_int;
    fn kz_model_range_histogram_fast(model: *const c_void, device: c_int, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, hist_out: *mut c_void) -> c_int;
    // tower taps and error profile: what the one-launch tower of (max_batch, dtype) stores at every range site, and its
    // deviation from exact f32 per site, out KzSiteError [n_sites]
    fn kz_model_tower_taps_path(model: *const c_void, max_batch: c_int, dtype: c_int, buf: *mut c_char, len: usize) -> c_int;
    fn kz_model_tower_taps(model: *const c_void, device: c_int, max_batch: c_int, dtype: c_int, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, site_first: c_int, n_sites: c_int, out: *mut f32) -> c_int;
    fn kz_model_error_profile(model: *const c_void, device: c_int, max_batch: c_int, dtype: c_int, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, out: *mut c_void) -> c_int;
    // int8 taps and error profile: every stored int8 image of the int8 tower of (max_batch, dtype 4 / 5 / 8), the f16 stream value
    // beside it, and per site their deviation from exact f32 with the clamp counts, out KzInt8SiteError [n_sites]
    fn kz_model_int8_taps_path(model: *const c_void, max_batch: c_int, dtype: c_int, buf: *mut c_char, len: usize) -> c_int;
    fn kz_model_int8_taps(model: *const c_void, device: c_int, max_batch: c_int, dtype: c_int, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, site_first: c_int, n_sites: c_int, image_out: *mut c_void, stream_out: *mut f32) -> c_int;
    fn kz_model_int8_error_profile(model: *const c_void, device: c_int, max_batch: c_int, dtype: c_int, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, out: *mut c_void) -> c_int;
    fn kz_engine_max_batch(engine: *const c_void) -> c_int;
    fn kz_engine_eval_dense(engine: *mut c_void, input_nchw: *const f32, batch: c_int, scalars_out: *mut f32, policy_out: *mut f32) -> c_int;
    fn kz_engine_eval_packed(engine: *mut c_void, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, scalars_out: *mut f32, policy_out: *mut f32) -> c_int;
    fn kz_engine_eval_packed_decoded(engine: *mut c_void, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, move_offsets: *const i64, move_indices: *const i32, values_out: *mut f32, probs_out: *mut f32) -> c_int;
    // asynchronous pair, slot in [0, KZ_ENGINE_SLOTS): inputs are copied to pinned staging before submit returns
    fn kz_engine_submit_packed(engine: *mut c_void, slot: c_int, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int) -> c_int;
    fn kz_engine_wait(engine: *mut c_void, slot: c_int, scalars_out: *mut f32, policy_out: *mut f32) -> c_int;
    fn kz_engine_wait_view(engine: *mut c_void, slot: c_int, scalars_out: *mut *const f32, policy_out: *mut *const f32) -> c_int;
    fn kz_engine_submit_packed_decoded(engine: *mut c_void, slot: c_int, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, move_offsets: *const i64, move_indices: *const i32) -> c_int;
    fn kz_engine_wait_decoded(engine: *mut c_void, slot: c_int, values_out: *mut *const f32, probs_out: *mut *const f32) -> c_int;
    // board symmetries inside the launch: two tables once, one id per board with every decoded submit (sym null: no symmetry)
    fn kz_engine_set_symmetries(engine: *mut c_void, n_sym: c_int, square_src: *const i32, policy_map: *const i32) -> c_int;
    fn kz_engine_eval_packed_decoded_sym(engine: *mut c_void, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, sym: *const u8, move_offsets: *const i64, move_indices: *const i32, values_out: *mut f32, probs_out: *mut f32) -> c_int;
    fn kz_engine_submit_packed_decoded_sym(engine: *mut c_void, slot: c_int, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, sym: *const u8, move_offsets: *const i64, move_indices: *const i32) -> c_int;
    // every board under every symmetry of the tables, averaged on the device: at most max_batch / n_sym boards per call
    fn kz_engine_eval_packed_decoded_avg(engine: *mut c_void, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, move_offsets: *const i64, move_indices: *const i32, values_out: *mut f32, probs_out: *mut f32) -> c_int;
    fn kz_engine_submit_packed_decoded_avg(engine: *mut c_void, slot: c_int, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, move_offsets: *const i64, move_indices: *const i32) -> c_int;
    // per-board status instead of a failing batch (status: u8 [batch], typed void in the header), and the exact-f32 range fallback
    fn kz_engine_wait_decoded_status(engine: *mut c_void, slot: c_int, values_out: *mut *const f32, probs_out: *mut *const f32, status_out: *mut *mut c_void) -> c_int;
    fn kz_engine_eval_packed_decoded_status(engine: *mut c_void, bits: *const u8, bits_stride: usize, scalars_in: *const f32, batch: c_int, sym: *const u8, move_offsets: *const i64, move_indices: *const i32, values_out: *mut f32, probs_out: *mut f32, status_out: *mut c_void) -> c_int;
    fn kz_engine_set_range_fallback(engine: *mut c_void, dtype: c_int) -> c_int;
    // the shadow audit: a sample of the decoded batches on a sibling engine of a <= 1e-4 dtype (out: a KzAuditStats, typed void in the header)
    fn kz_engine_set_audit(engine: *mut c_void, dtype: c_int, period: c_int, boards: c_int) -> c_int;
    fn kz_engine_audit_stats(engine: *mut c_void, out: *mut c_void, reset: c_int) -> c_int;
    // device-resident entry points and helpers (benchmarks and parity tests; the server does not need them)
    fn kz_engine_enqueue_packed_device(engine: *mut c_void, d_bits: *const c_void, bits_stride: usize, d_scalars_in: *const c_void, batch: c_int, d_scalars_out: *mut c_void, d_policy_out: *mut c_void) -> c_int;
    fn kz_engine_enqueue_dense_device(engine: *mut c_void, d_input_nchw: *const c_void, batch: c_int, d_scalars_out: *mut c_void, d_policy_out: *mut c_void) -> c_int;
    fn kz_engine_synchronize(engine: *mut c_void) -> c_int;
    fn kz_device_malloc(device: c_int, bytes: usize, out: *mut *mut c_void) -> c_int;
    fn kz_device_free(device: c_int, ptr: *mut c_void) -> c_int;
    fn kz_memcpy_h2d(device: c_int, dst: *mut c_void, src: *const c_void, bytes: usize) -> c_int;
    fn kz_memcpy_d2h(device: c_int, dst: *mut c_void, src: *const c_void, bytes: usize) -> c_int;
    fn kz_device_synchronize(device: c_int) -> c_int;
    fn kz_engine_set_profiling(engine: *mut c_void, enable: c_int) -> c_int;
    fn kz_engine_kernel_time(engine: *mut c_void, prefix: *const c_char, total_ms: *mut f64, launches: *mut i64) -> c_int;
    fn kz_engine_tower_path(engine: *const c_void) -> *const c_char;
    fn kz_engine_launch_geometry(engine: *const c_void, batch: c_int, workgroups: *mut c_int, boards_per_workgroup: *mut c_int) -> c_int;
    fn kz_engine_read_activation(engine: *mut c_void, name: *const c_char, batch: c_int, out_nchw: *mut f32) -> c_int;
}

/// The reference panics on every executor error (`unwrap()` cudnn.rs:70,78); keep that behaviour.
fn check(rc: c_int) {
    if rc != 0 {
        let msg = unsafe { CStr::from_ptr(kz_last_error()) }.to_string_lossy().into_owned();
        panic!("kzhip: {}", msg);
    }
}

pub fn hip_device_count() -> usize {
    let mut n = 0;
    check(unsafe { kz_device_count(&mut n) });
    n as usize
}

/// What replaces `kn_cuda_sys::wrapper::handle::CudaDevice` at the server seam (`ZeroSpecialization::Device`,
/// INTEGRATION.md §1): a HIP device ordinal.  `CudaDevice::all()` (server.rs:49) -> `HipDevice::all()`,
/// `CudaDevice::new(d).unwrap()` (server.rs:51) -> `HipDevice::new(d)`.
#[derive(Debug, Copy, Clone, Eq, PartialEq, Hash)]
pub struct HipDevice(pub usize);

impl HipDevice {
    pub fn all() -> Vec<HipDevice> {
        (0..hip_device_count()).map(HipDevice).collect()
    }
    pub fn new(index: i32) -> HipDevice {
        assert!(index >= 0 && (index as usize) < hip_device_count(), "No HIP device {}", index);
        HipDevice(index as usize)
    }
    pub fn pci_bus_id(self) -> String {
        let mut buf = [0 as c_char; 64];
        check(unsafe { kz_device_pci_bus_id(self.0 as c_int, buf.as_mut_ptr(), buf.len()) });
        unsafe { CStr::from_ptr(buf.as_ptr()) }.to_string_lossy().into_owned()
    }
}

/// Arithmetic of the engine, a start-up choice (environment variable `KZ_HIP_DTYPE`, read once by
/// `HipSpecialization`).  The reference's executor is f32 only (`DTensor::F32`, cudnn.rs:73) and the stated parity is
/// 1e-4, so the DEFAULT is the fastest path that keeps it: `KZ_DTYPE_F32_SPLIT16` where the network's shape allows,
/// else `KZ_DTYPE_F32`.  `f16` (3 x faster again, tolerance 5e-3 of the output scale, range +-65504 with overflow
/// reported as an error) is opt-in, and so is `bf16` (`KZ_DTYPE_BF16`: the f16 rate with f32's range — no overflow to
/// report — at 8 significant bits; the one-launch ResTower shapes only, anything else fails at engine creation).
#[derive(Debug, Copy, Clone, Eq, PartialEq)]
pub enum HipDtype {
    Parity,
    F32,
    F16,
    Bf16,
}

impl HipDtype {
    pub fn from_env() -> HipDtype {
        match std::env::var("KZ_HIP_DTYPE").as_deref() {
            Err(_) | Ok("parity") | Ok("f32split16") => HipDtype::Parity,
            Ok("f32") => HipDtype::F32,
            Ok("f16") => HipDtype::F16,
            Ok("bf16") => HipDtype::Bf16,
            Ok(other) => panic!("KZ_HIP_DTYPE must be parity, f32, f16 or bf16, got '{}'", other),
        }
    }
    fn resolve(self, model: &HipModel) -> c_int {
        match self {
            HipDtype::F32 => KZ_DTYPE_F32,
            HipDtype::F16 => KZ_DTYPE_F16,
            HipDtype::Bf16 => KZ_DTYPE_BF16,
            HipDtype::Parity => {
                if unsafe { kz_model_supports_dtype(model.ptr, KZ_DTYPE_F32_SPLIT16) } == 1 {
                    KZ_DTYPE_F32_SPLIT16
                } else {
                    KZ_DTYPE_F32
                }
            }
        }
    }
}

/// Host-side parsed model: the `G` of `ZeroSpecialization` (what `Arc<Graph>` is for `AlphaZeroSpecialization`).
pub struct HipModel {
    ptr: *mut c_void,
    pub info: KzModelInfo,
}

// kz_model is immutable and thread-safe (include/kz_hip.h)
unsafe impl Send for HipModel {}
unsafe impl Sync for HipModel {}

impl HipModel {
    /// `path`: the ONNX file the trainer writes (python/lib/save_onnx.py); `input_scalar_count`: the mapper's, the
    /// graph itself does not say which of its input planes are broadcast scalars.
    pub fn load(path: &str, input_scalar_count: usize) -> Self {
        let c_path = CString::new(path).unwrap();
        let mut ptr = std::ptr::null_mut();
        check(unsafe { kz_model_load_onnx(c_path.as_ptr(), input_scalar_count as c_int, &mut ptr) });
        let mut info = KzModelInfo::default();
        check(unsafe { kz_model_get_info(ptr, &mut info) });
        HipModel { ptr, info }
    }

    fn adopt(ptr: *mut c_void) -> Self {
        let mut info = KzModelInfo::default();
        check(unsafe { kz_model_get_info(ptr, &mut info) });
        HipModel { ptr, info }
    }

    /// The same function with a residual stream 2^-k times as large (`kz_model_stream_shift`): f16 and the parity arithmetic
    /// for a network whose stream leaves +-65504.  k in [-24, 24]; panics where the library refuses.
    pub fn stream_shift(&self, k: i32) -> HipModel {
        let mut ptr = std::ptr::null_mut();
        check(unsafe { kz_model_stream_shift(self.ptr, k as c_int, &mut ptr) });
        HipModel::adopt(ptr)
    }

    /// `KZ_HIP_STREAM_SHIFT=<k>` (default 0; read here, never by the library), what `load_graph` applies to every network it
    /// loads: choose k from a range profile of the network on its own positions (`range_profile`, `shift_for`;
    /// tools/range_profile.py prints both) — or let `KZ_HIP_STREAM_SHIFT=auto[:<headroom bits>]` choose it per network
    /// (`auto_stream_shift` on the process-wide `position_sample()`, which every `HipNetwork` then feeds).  The first
    /// network of a run, with no positions sampled yet, gets k = 0: pair `auto` with `KZ_HIP_RANGE_FALLBACK=1` for it.
    pub fn stream_shift_from_env(self) -> HipModel {
        match StreamShift::from_env() {
            StreamShift::Fixed(0) => self,
            StreamShift::Fixed(k) => self.stream_shift(k),
            StreamShift::Auto(headroom_bits) => {
                let (shifted, k, max_abs, boards) = self.auto_stream_shift(position_sample(), headroom_bits);
                eprintln!("kz_hip stream shift: k = {} (max |x| {:e} on {} sampled boards, {} bits of headroom)", k, max_abs, boards, headroom_bits);
                shifted.unwrap_or(self)
            }
        }
    }

    /// The shift this network needs on the positions of `sample` (the C++ mirror's `HipModel::auto_stream_shift`):
    /// `range_profile_fast` on a snapshot — on the device whose executor offered last —, m = the largest board_max,
    /// k = `shift_for(m, headroom_bits)`.  Returns (`stream_shift(k)`, or None for k == 0: keep this model; k; m; boards
    /// profiled).  An empty sample gives k = 0 with boards = 0.  Panics when m is +inf: a network that overflows f32 is not
    /// a shift's business.
    pub fn auto_stream_shift(&self, sample: &PositionSample, headroom_bits: i32) -> (Option<HipModel>, i32, f32, usize) {
        let snap = sample.snapshot();
        if snap.boards == 0 {
            return (None, 0, 0.0, 0);
        }
        assert_eq!((snap.bits_bytes, snap.n_scalar), (self.info.bits_bytes as usize, self.info.input_scalar_channels.max(0) as usize), "auto_stream_shift: the sample holds boards of another shape than this model's");
        let (_, board_max) = self.range_profile_fast(snap.device, &snap.bits, snap.bits_bytes, &snap.scalars, snap.boards);
        let max_abs = board_max.iter().cloned().fold(0f32, f32::max);
        assert!(max_abs.is_finite(), "auto_stream_shift: the residual stream is not finite in exact f32 on the {} sampled boards: no shift brings such a network into range", snap.boards);
        let k = shift_for(max_abs, headroom_bits);
        (if k == 0 { None } else { Some(self.stream_shift(k)) }, k, max_abs, snap.boards)
    }

    /// The names of the range profile's sites, in order (`kz_model_range_sites`, `kz_model_range_site_name`).
    pub fn range_sites(&self) -> Vec<String> {
        let mut n = 0;
        check(unsafe { kz_model_range_sites(self.ptr, &mut n) });
        (0..n)
            .map(|site| {
                let mut buf = [0 as c_char; 32];
                check(unsafe { kz_model_range_site_name(self.ptr, site, buf.as_mut_ptr(), buf.len()) });
                unsafe { CStr::from_ptr(buf.as_ptr()) }.to_string_lossy().into_owned()
            })
            .collect()
    }

    /// max |x| of every stored tower tensor on these packed boards, in exact f32 on `device` (`kz_model_range_profile`):
    /// (per site over all boards, per board over the sites a shift moves).
    pub fn range_profile(&self, device: HipDevice, bits: &[u8], bits_stride: usize, scalars_in: &[f32], batch: usize) -> (Vec<f32>, Vec<f32>) {
        let mut n = 0;
        check(unsafe { kz_model_range_sites(self.ptr, &mut n) });
        assert!(bits.len() >= batch * bits_stride && scalars_in.len() >= batch * self.info.input_scalar_channels.max(0) as usize);
        let (mut site_max, mut board_max) = (vec![0f32; n as usize], vec![0f32; batch]);
        check(unsafe {
            kz_model_range_profile(self.ptr, device.0 as c_int, bits.as_ptr(), bits_stride, scalars_in.as_ptr(), batch as c_int, site_max.as_mut_ptr(), board_max.as_mut_ptr())
        });
        (site_max, board_max)
    }

    /// The same profile inside the one-launch exact-f32 tower where that kernel takes the network — tens of thousands of
    /// boards per second — and exactly `range_profile` elsewhere (`kz_model_range_profile_fast`).
    pub fn range_profile_fast(&self, device: HipDevice, bits: &[u8], bits_stride: usize, scalars_in: &[f32], batch: usize) -> (Vec<f32>, Vec<f32>) {
        let mut n = 0;
        check(unsafe { kz_model_range_sites(self.ptr, &mut n) });
        assert!(bits.len() >= batch * bits_stride && scalars_in.len() >= batch * self.info.input_scalar_channels.max(0) as usize);
        let (mut site_max, mut board_max) = (vec![0f32; n as usize], vec![0f32; batch]);
        check(unsafe {
            kz_model_range_profile_fast(self.ptr, device.0 as c_int, bits.as_ptr(), bits_stride, scalars_in.as_ptr(), batch as c_int, site_max.as_mut_ptr(), board_max.as_mut_ptr())
        });
        (site_max, board_max)
    }

    /// How many stored values of every site lie in each binade, counted in exact f32 on `device`: `[n_sites][KZ_RANGE_BINS]`
    /// flat, every site summing to batch * h * w * tower_channels (`kz_model_range_histogram_fast`: inside the one-launch tower where
    /// `range_profile_fast_path` says so; `fast = false`: `kz_model_range_histogram`, per layer).  `shift_report` reads it.
    pub fn range_histogram(&self, device: HipDevice, bits: &[u8], bits_stride: usize, scalars_in: &[f32], batch: usize, fast: bool) -> Vec<u64> {
        let mut n = 0;
        check(unsafe { kz_model_range_sites(self.ptr, &mut n) });
        assert!(bits.len() >= batch * bits_stride && scalars_in.len() >= batch * self.info.input_scalar_channels.max(0) as usize);
        let mut hist = vec![0u64; n as usize * KZ_RANGE_BINS];
        let out = hist.as_mut_ptr() as *mut c_void;
        check(unsafe {
            if fast {
                kz_model_range_histogram_fast(self.ptr, device.0 as c_int, bits.as_ptr(), bits_stride, scalars_in.as_ptr(), batch as c_int, out)
            } else {
                kz_model_range_histogram(self.ptr, device.0 as c_int, bits.as_ptr(), bits_stride, scalars_in.as_ptr(), batch as c_int, out)
            }
        });
        hist
    }

    /// (workgroups, boards per workgroup) an engine of (max_batch, dtype) reports for `batch` (`kz_model_launch_geometry`; no GPU).
    pub fn launch_geometry(&self, max_batch: usize, dtype: i32, batch: usize) -> (usize, usize) {
        let (mut wgs, mut per) = (0, 0);
        check(unsafe { kz_model_launch_geometry(self.ptr, max_batch as c_int, dtype as c_int, batch as c_int, &mut wgs, &mut per) });
        (wgs as usize, per as usize)
    }

    /// The kernel a tap call runs: `kz_model_plan(max_batch, dtype)`'s tower without "+heads" (`kz_model_tower_taps_path`; no GPU).
    pub fn tower_taps_path(&self, max_batch: usize, dtype: i32) -> String {
        let mut buf = [0 as c_char; 64];
        check(unsafe { kz_model_tower_taps_path(self.ptr, max_batch as c_int, dtype as c_int, buf.as_mut_ptr(), buf.len()) });
        unsafe { CStr::from_ptr(buf.as_ptr()) }.to_string_lossy().into_owned()
    }

    /// What the one-launch tower of an engine of (max_batch, dtype) stores at the range sites `site_first .. site_first + n_sites`
    /// on these packed boards, as the kernel rounds it (`kz_model_tower_taps`): f32 `[n_sites][batch][C][H][W]` flat.
    pub fn tower_taps(&self, device: HipDevice, max_batch: usize, dtype: i32, bits: &[u8], bits_stride: usize, scalars_in: &[f32], batch: usize, site_first: usize, n_sites: usize) -> Vec<f32> {
        assert!(bits.len() >= batch * bits_stride && scalars_in.len() >= batch * self.info.input_scalar_channels.max(0) as usize);
        let per_site = batch * self.info.tower_channels as usize * self.info.board_h as usize * self.info.board_w as usize;
        let mut out = vec![0f32; n_sites * per_site];
        check(unsafe {
            kz_model_tower_taps(self.ptr, device.0 as c_int, max_batch as c_int, dtype as c_int, bits.as_ptr(), bits_stride, scalars_in.as_ptr(), batch as c_int, site_first as c_int, n_sites as c_int, out.as_mut_ptr())
        });
        out
    }

    /// The kernel an int8 tap call runs, "tower_resident_i8" or "board_conv_i8" (`kz_model_int8_taps_path`; no GPU).
    pub fn int8_taps_path(&self, max_batch: usize, dtype: i32) -> String {
        let mut buf = [0 as c_char; 64];
        check(unsafe { kz_model_int8_taps_path(self.ptr, max_batch as c_int, dtype as c_int, buf.as_mut_ptr(), buf.len()) });
        unsafe { CStr::from_ptr(buf.as_ptr()) }.to_string_lossy().into_owned()
    }

    /// What the int8 tower of an engine of (max_batch, dtype) stores at the range sites `site_first .. site_first + n_sites` on
    /// these packed boards (`kz_model_int8_taps`): the images' q and the f16 stream values, `[n_sites][batch][C][H][W]` flat each.
    pub fn int8_taps(&self, device: HipDevice, max_batch: usize, dtype: i32, bits: &[u8], bits_stride: usize, scalars_in: &[f32], batch: usize, site_first: usize, n_sites: usize) -> (Vec<i8>, Vec<f32>) {
        assert!(bits.len() >= batch * bits_stride && scalars_in.len() >= batch * self.info.input_scalar_channels.max(0) as usize);
        let per_site = batch * self.info.tower_channels as usize * self.info.board_h as usize * self.info.board_w as usize;
        let (mut image, mut stream) = (vec![0i8; n_sites * per_site], vec![0f32; n_sites * per_site]);
        check(unsafe {
            kz_model_int8_taps(self.ptr, device.0 as c_int, max_batch as c_int, dtype as c_int, bits.as_ptr(), bits_stride, scalars_in.as_ptr(), batch as c_int, site_first as c_int, n_sites as c_int, image.as_mut_ptr() as *mut c_void, stream.as_mut_ptr())
        });
        (image, stream)
    }

    /// Per range site, the error of that int8 tower's images and stream values against exact f32 and the clamp counts (`kz_model_int8_error_profile`).
    pub fn int8_error_profile(&self, device: HipDevice, max_batch: usize, dtype: i32, bits: &[u8], bits_stride: usize, scalars_in: &[f32], batch: usize) -> Vec<KzInt8SiteError> {
        let mut n = 0;
        check(unsafe { kz_model_range_sites(self.ptr, &mut n) });
        assert!(bits.len() >= batch * bits_stride && scalars_in.len() >= batch * self.info.input_scalar_channels.max(0) as usize);
        let mut out = vec![KzInt8SiteError::default(); n as usize];
        check(unsafe {
            kz_model_int8_error_profile(self.ptr, device.0 as c_int, max_batch as c_int, dtype as c_int, bits.as_ptr(), bits_stride, scalars_in.as_ptr(), batch as c_int, out.as_mut_ptr() as *mut c_void)
        });
        out
    }

    /// Per range site, how far that tower's stored tensors are from exact f32 on these boards (`kz_model_error_profile`).
    pub fn error_profile(&self, device: HipDevice, max_batch: usize, dtype: i32, bits: &[u8], bits_stride: usize, scalars_in: &[f32], batch: usize) -> Vec<KzSiteError> {
        let mut n = 0;
        check(unsafe { kz_model_range_sites(self.ptr, &mut n) });
        assert!(bits.len() >= batch * bits_stride && scalars_in.len() >= batch * self.info.input_scalar_channels.max(0) as usize);
        let mut out = vec![KzSiteError::default(); n as usize];
        check(unsafe {
            kz_model_error_profile(self.ptr, device.0 as c_int, max_batch as c_int, dtype as c_int, bits.as_ptr(), bits_stride, scalars_in.as_ptr(), batch as c_int, out.as_mut_ptr() as *mut c_void)
        });
        out
    }

    /// Where `range_profile_fast` runs: "tower_resident_f32" or "conv_igemm_f32" (`kz_model_range_profile_fast_path`; no GPU).
    pub fn range_profile_fast_path(&self) -> String {
        let mut buf = [0 as c_char; 32];
        check(unsafe { kz_model_range_profile_fast_path(self.ptr, buf.as_mut_ptr(), buf.len()) });
        unsafe { CStr::from_ptr(buf.as_ptr()) }.to_string_lossy().into_owned()
    }
}

/// `KZ_HIP_STREAM_SHIFT`: `<k>` (an integer in [-24, 24]; unset = 0, the network as trained) or `auto[:<headroom bits>]`
/// (default 2 bits).
#[derive(Debug, Copy, Clone, Eq, PartialEq)]
pub enum StreamShift {
    Fixed(i32),
    Auto(i32),
}

impl StreamShift {
    pub fn parse(v: &str) -> StreamShift {
        fn usage(v: &str) -> ! {
            panic!("KZ_HIP_STREAM_SHIFT must be an integer in [-24, 24] or auto[:<headroom bits>], got '{}'", v)
        }
        if v == "auto" {
            return StreamShift::Auto(2);
        }
        if let Some(bits) = v.strip_prefix("auto:") {
            return StreamShift::Auto(bits.parse::<i32>().unwrap_or_else(|_| usage(v)));
        }
        StreamShift::Fixed(v.parse::<i32>().unwrap_or_else(|_| usage(v)))
    }
    pub fn from_env() -> StreamShift {
        match std::env::var("KZ_HIP_STREAM_SHIFT") {
            Err(_) => StreamShift::Fixed(0),
            Ok(v) => StreamShift::parse(&v),
        }
    }
}

/// The most recent packed boards this process's executors have evaluated (the C++ mirror's host/position_sample.hpp is the
/// tested statement): `offer` keeps the first `take` boards of every `period`-th call — the audit's deterministic prefix
/// rule, a memcpy — in a ring of `capacity` boards; `snapshot` copies it out, oldest first.  One instance for all executors,
/// so that a model is shifted once: a k per executor thread would mean a device weight copy per thread.
pub struct PositionSample {
    capacity: usize,
    period: usize,
    take: usize,
    inner: Mutex<SampleRing>,
}

#[derive(Default)]
struct SampleRing {
    bits_bytes: usize,
    n_scalar: usize,
    head: usize,
    size: usize,
    calls: usize,
    device: usize,
    bits: Vec<u8>,
    scalars: Vec<f32>,
}

pub struct SampleSnapshot {
    pub bits: Vec<u8>,
    pub scalars: Vec<f32>,
    pub boards: usize,
    pub bits_bytes: usize,
    pub n_scalar: usize,
    /// the device of the executor that offered last
    pub device: HipDevice,
}

impl PositionSample {
    pub fn with_capacity(capacity: usize, period: usize, take: usize) -> Self {
        assert!(capacity >= 1 && period >= 1 && take >= 1);
        PositionSample { capacity, period, take, inner: Mutex::new(SampleRing::default()) }
    }

    /// `batch` packed boards as an engine takes them; boards of another shape than the ones held (another game) empty the ring.
    pub fn offer(&self, device: HipDevice, bits: &[u8], bits_bytes: usize, scalars: &[f32], n_scalar: usize, batch: usize) {
        let mut r = self.inner.lock().unwrap();
        if r.bits_bytes != bits_bytes || r.n_scalar != n_scalar || r.bits.len() != self.capacity * bits_bytes {
            *r = SampleRing { bits_bytes, n_scalar, bits: vec![0; self.capacity * bits_bytes], scalars: vec![0.0; self.capacity * n_scalar], ..SampleRing::default() };
        }
        r.device = device.0;
        r.calls += 1;
        if (r.calls - 1) % self.period != 0 {
            return;
        }
        for b in 0..self.take.min(batch) {
            let at = (r.head + r.size) % self.capacity;
            r.bits[at * bits_bytes..(at + 1) * bits_bytes].copy_from_slice(&bits[b * bits_bytes..(b + 1) * bits_bytes]);
            r.scalars[at * n_scalar..(at + 1) * n_scalar].copy_from_slice(&scalars[b * n_scalar..(b + 1) * n_scalar]);
            if r.size < self.capacity {
                r.size += 1;
            } else {
                r.head = (r.head + 1) % self.capacity;
            }
        }
    }

    pub fn snapshot(&self) -> SampleSnapshot {
        let r = self.inner.lock().unwrap();
        let (bb, ns) = (r.bits_bytes, r.n_scalar);
        let mut snap = SampleSnapshot { bits: Vec::with_capacity(r.size * bb), scalars: Vec::with_capacity(r.size * ns), boards: r.size, bits_bytes: bb, n_scalar: ns, device: HipDevice(r.device) };
        for i in 0..r.size {
            let at = (r.head + i) % self.capacity;
            snap.bits.extend_from_slice(&r.bits[at * bb..(at + 1) * bb]);
            snap.scalars.extend_from_slice(&r.scalars[at * ns..(at + 1) * ns]);
        }
        snap
    }
}

/// `kz_site_error` (include/kz_hip.h): one range site of `HipModel::error_profile`, 48 bytes.
#[repr(C)]
#[derive(Debug, Default, Copy, Clone, PartialEq)]
pub struct KzSiteError {
    pub max_abs_err: f64,
    pub sum_sq_err: f64,
    pub sum_sq_ref: f64,
    pub max_abs_ref: f64,
    pub count: u64,
    pub nonfinite: u64,
}

/// `kz_int8_site_error` (include/kz_hip.h): one range site of `HipModel::int8_error_profile`, 120 bytes.
#[repr(C)]
#[derive(Debug, Default, Copy, Clone, PartialEq)]
pub struct KzInt8SiteError {
    pub image: KzSiteError,
    pub stream: KzSiteError,
    pub at_clamp: u64,
    pub ref_beyond: u64,
    pub exponent: i32,
    pub reserved: i32,
}

/// The bins of `HipModel::range_histogram` (include/kz_hip.h): 0 is +-0, 95 inf or NaN, b in 1..=94 the binade E = b - 51
/// with the two ends clamped.
pub const KZ_RANGE_BINS: usize = 96;

/// What a stream shift of k does to the stored values of one site of a range histogram (`shift_report`).
#[derive(Debug, Clone, Copy, Default, PartialEq, Eq)]
pub struct ShiftReport {
    pub total: u64,
    pub zero: u64,
    pub nonfinite: u64,
    /// E' >= 16: beyond f16
    pub f16_over: u64,
    /// E' = 15: the binade that holds 65504 .. 65536
    pub f16_top: u64,
    /// -25 <= E' <= -15
    pub f16_subnormal: u64,
    /// E' < -25
    pub f16_flushed: u64,
    /// E' <= -3: the lo half of a split16 pair is subnormal or gone
    pub split_lo_subnormal: u64,
    /// the two end bins (E <= -50, E >= 43) as they are: for every k in [-24, 24] they lie in `f16_flushed` (and
    /// `split_lo_subnormal`) and in `f16_over`, so nothing is guessed
    pub clamped_low: u64,
    pub clamped_high: u64,
}

/// Per site of `hist` (`[n_sites][KZ_RANGE_BINS]` flat, as `HipModel::range_histogram` returns it): E' = E - k on the shifted sites, E' = E on the last one.  Integer arithmetic only; the library
/// reports, the caller decides, as for `shift_for`.
pub fn shift_report(hist: &[u64], k: i32) -> Vec<ShiftReport> {
    assert!(!hist.is_empty() && hist.len() % KZ_RANGE_BINS == 0, "shift_report: hist must be [n_sites][96]");
    assert!((-24..=24).contains(&k), "shift_report: k = {} out of range [-24, 24]", k);
    let n = hist.len() / KZ_RANGE_BINS;
    hist.chunks(KZ_RANGE_BINS)
        .enumerate()
        .map(|(site, row)| {
            let shift = if site + 1 < n { k } else { 0 };
            let mut r = ShiftReport { total: row.iter().sum(), zero: row[0], nonfinite: row[KZ_RANGE_BINS - 1], clamped_low: row[1], clamped_high: row[KZ_RANGE_BINS - 2], ..Default::default() };
            for b in 1..KZ_RANGE_BINS - 1 {
                let e = b as i32 - 51 - shift; // (bin 1: at most this; bin 94: at least this: the classes hold for both)
                if e >= 16 {
                    r.f16_over += row[b];
                }
                if e == 15 {
                    r.f16_top += row[b];
                }
                if (-25..=-15).contains(&e) {
                    r.f16_subnormal += row[b];
                }
                if e < -25 {
                    r.f16_flushed += row[b];
                }
                if e <= -3 {
                    r.split_lo_subnormal += row[b];
                }
            }
            r
        })
        .collect()
}

/// The sample `KZ_HIP_STREAM_SHIFT=auto` profiles: process-wide, fed by every `HipNetwork` (the first 64 boards of every
/// batch, the most recent 16384 kept: 2 MB for chess).
pub fn position_sample() -> &'static PositionSample {
    static SAMPLE: OnceLock<PositionSample> = OnceLock::new();
    SAMPLE.get_or_init(|| PositionSample::with_capacity(16384, 1, 64))
}

/// The k of `HipModel::stream_shift` for a stream whose shifted sites reach `max_abs` (include/kz_hip.h):
/// k = max(0, ceil(log2(max_abs / 65504)) + headroom_bits), computed without a floating-point logarithm.
pub fn shift_for(max_abs: f32, headroom_bits: i32) -> i32 {
    assert!(max_abs.is_finite() && max_abs >= 0.0, "shift_for: max_abs must be finite and non-negative, got {}", max_abs);
    if max_abs == 0.0 {
        return 0;
    }
    // the smallest e with max_abs <= 65504 * 2^e
    let ratio = max_abs as f64 / 65504.0;
    let mut e = 0;
    while ratio > (2.0f64).powi(e) {
        e += 1;
    }
    while e > -200 && ratio <= (2.0f64).powi(e - 1) {
        e -= 1;
    }
    (e + headroom_bits).max(0)
}

impl Drop for HipModel {
    fn drop(&mut self) {
        unsafe { kz_model_free(self.ptr) }
    }
}

/// The symmetries of a game as the engine takes them (`kz_engine_set_symmetries`): `square_src[sym][s]` is the square of
/// the board whose planes the mapped board has at `s`, `policy_map[sym][i]` the policy index of the image of the move with
/// index `i` (-1: the mapped board has no such move).  Built once per game from `B::Symmetry::all()`, `map_coord` /
/// `map_move` and the mapper's `move_to_index` / `index_to_move`; the C++ mirror's `d4_tables` (host/symmetry.hpp) is the
/// tested statement for Ataxx and Go.
pub struct SymmetryTables {
    pub n_sym: usize,
    pub square_src: Vec<i32>,
    pub policy_map: Vec<i32>,
}

pub struct HipNetwork<B: Board, M: BoardMapper<B>> {
    mapper: M,
    max_batch_size: usize,
    engine: *mut c_void,
    _model: Arc<HipModel>,

    bits: Vec<u8>,
    scalars_in: Vec<f32>,
    scalars_out: Vec<f32>,
    policy_out: Vec<f32>,
    /// boards of the batches in flight, oldest first (decode_output needs their available moves); with the
    /// device-side decode the boards are dropped at submit and the CSR offsets of their move lists are kept instead
    pending: VecDeque<(usize, Vec<B>, Vec<i64>)>,
    next_slot: usize,
    /// `KZ_HIP_DECODE` (default "device"): decode_output's gather + softmax on the GPU
    device_decode: bool,
    move_offsets: Vec<i64>,
    move_indices: Vec<i32>,
    /// `eval_random_symmetries` inside the launch (`new_with_symmetries`): the number of symmetries (0: off), the source
    /// of the ids and the ids of the batch being submitted
    n_sym: usize,
    sym_rng: Option<Box<dyn rand::RngCore + Send>>,
    sym_ids: Vec<u8>,
    /// `AverageSymmetryNetwork` inside the engine (`new_with_average_symmetries`): every board under all `n_sym`
    /// symmetries, averaged on the device; a batch is then at most `max_batch_size / n_sym` boards per engine call
    average_symmetries: bool,
    /// `KZ_HIP_RANGE_FALLBACK=1` (default off; read here, never by the library): boards of an f16 / split16 batch whose
    /// activations leave the f16 range are re-evaluated in exact f32 inside the engine (`kz_engine_set_range_fallback`)
    /// instead of panicking the executor; how many boards that has happened to so far
    pub fell_back_boards: u64,
    /// `KZ_HIP_AUDIT=<period>[:<boards>[:f32|split16]]` (default off; read here, never by the library): the first `boards`
    /// (default 16) boards of every `period`-th decoded batch also run on a sibling engine in a <= 1e-4 arithmetic (default
    /// split16 where the model has it and the engine is not split16 itself, else f32) and the deviation is accumulated
    /// (`kz_engine_set_audit`); `drop` prints the totals to stderr in one line, i.e. once per network generation
    audit: bool,
    /// `KZ_HIP_PREP_THREADS` (default 0) + 1 ranges of a batch, each prepared by one thread (`prepare`)
    ranges: Vec<PrepRange>,
    /// `KZ_HIP_STREAM_SHIFT=auto`: the boards `prepare` has just packed are offered to `position_sample()`, from this device
    sample_from: Option<HipDevice>,
    ph: PhantomData<B>,
}

/// What one thread prepares for its contiguous range of a batch's boards.
#[derive(Default)]
struct PrepRange {
    scalars: Vec<f32>,
    /// available moves per board
    counts: Vec<i64>,
    /// `move_to_index` of every available move, board after board
    indices: Vec<i32>,
}

/// `encode_input` of the boards of one range into `bits` (that range's part of the staging) and `out.scalars`, and — with
/// the decode on the device — `move_to_index` of every available move (what decode_output computes per board,
/// common.rs:77-81, hoisted in front of the evaluation).
fn prep_range<B: Board, M: BoardMapper<B>>(mapper: M, boards: &[&B], bits: &mut [u8], with_moves: bool, out: &mut PrepRange) {
    let bool_count = mapper.input_bool_len();
    let bits_bytes = (bool_count + 7) / 8;
    let policy_len = mapper.policy_len();
    out.scalars.clear();
    out.counts.clear();
    out.indices.clear();
    let mut buffer = BitBuffer::new(bool_count);
    for (bi, &board) in boards.iter().enumerate() {
        buffer.clear();
        // packed encode: exactly what BinaryOutput stores per position (binary_output.rs:210-256)
        mapper.encode_input(&mut buffer, &mut out.scalars, board);
        assert_eq!(bool_count, buffer.len());
        bits[bi * bits_bytes..(bi + 1) * bits_bytes].copy_from_slice(buffer.storage());
        if !with_moves {
            continue;
        }
        let before = out.indices.len();
        // `available_moves()` is an InternalIterator behind a Result (Err = the game is over: no moves, an empty
        // policy — decode_output's `map_or(vec![], ..)`, common.rs:77)
        if let Ok(moves) = board.available_moves() {
            let indices = &mut out.indices;
            moves.for_each(|mv| {
                let index = mapper.move_to_index(board, mv);
                assert!(index < policy_len);
                indices.push(index as i32);
            });
        }
        out.counts.push((out.indices.len() - before) as i64);
    }
}

// one engine per executor thread; it is moved into that thread once (executor.rs:320-342)
unsafe impl<B: Board, M: BoardMapper<B>> Send for HipNetwork<B, M> {}

impl<B: Board, M: BoardMapper<B>> HipNetwork<B, M> {
    /// Mirrors `CudaNetwork::new(mapper, &graph, max_batch_size, device)` (cudnn.rs:29-43).
    pub fn new(mapper: M, model: Arc<HipModel>, max_batch_size: usize, device: HipDevice, dtype: HipDtype) -> Self {
        // check_graph_shapes (network/common.rs:165-198)
        let info = model.info;
        let [c, h, w] = mapper.input_full_shape();
        assert_eq!(
            [info.input_channels as usize, info.board_h as usize, info.board_w as usize],
            [c, h, w],
            "Input shape mismatch between model and mapper"
        );
        assert_eq!(info.input_scalar_channels as usize, mapper.input_scalar_count());
        assert_eq!(info.policy_len as usize, mapper.policy_len(), "Wrong policy shape");

        let mut engine = std::ptr::null_mut();
        let dtype = dtype.resolve(&model);
        check(unsafe { kz_engine_create(model.ptr, device.0 as c_int, max_batch_size as c_int, dtype, &mut engine) });
        match std::env::var("KZ_HIP_RANGE_FALLBACK").as_deref() {
            Err(_) | Ok("0") => {}
            // (an exact-f32 engine has no f16 range to fall back from: the library refuses it, so it is not asked)
            Ok("1") => if dtype != KZ_DTYPE_F32 { check(unsafe { kz_engine_set_range_fallback(engine, KZ_DTYPE_F32) }) },
            Ok(other) => panic!("KZ_HIP_RANGE_FALLBACK must be 0 or 1, got '{}'", other),
        }
        let audit = match std::env::var("KZ_HIP_AUDIT") {
            Err(_) => false,
            Ok(v) => {
                fn usage(v: &str) -> ! {
                    panic!("KZ_HIP_AUDIT must be <period>[:<boards>[:f32|split16]], got '{}'", v)
                }
                let mut parts = v.split(':');
                let period: c_int = parts.next().and_then(|p| p.trim().parse().ok()).unwrap_or_else(|| usage(&v));
                let boards: c_int = parts.next().map_or(16, |b| b.trim().parse().unwrap_or_else(|_| usage(&v)));
                let split16_fits = dtype != KZ_DTYPE_F32_SPLIT16 && unsafe { kz_model_supports_dtype(model.ptr, KZ_DTYPE_F32_SPLIT16) } == 1;
                let against = match parts.next() {
                    None => if split16_fits { KZ_DTYPE_F32_SPLIT16 } else { KZ_DTYPE_F32 },
                    Some("f32") => KZ_DTYPE_F32,
                    Some("split16") => KZ_DTYPE_F32_SPLIT16,
                    Some(_) => usage(&v),
                };
                if parts.next().is_some() {
                    usage(&v);
                }
                // (a sample larger than the sibling engine holds is the sibling's whole batch)
                let boards = boards.min(max_batch_size.min(64) as c_int);
                check(unsafe { kz_engine_set_audit(engine, against, period, boards) });
                true
            }
        };

        HipNetwork {
            mapper,
            max_batch_size,
            engine,
            bits: vec![0; max_batch_size * info.bits_bytes as usize],
            scalars_in: Vec::with_capacity(max_batch_size * mapper.input_scalar_count()),
            scalars_out: vec![0.0; max_batch_size * 5],
            policy_out: vec![0.0; max_batch_size * mapper.policy_len()],
            _model: model,
            pending: VecDeque::new(),
            next_slot: 0,
            device_decode: match std::env::var("KZ_HIP_DECODE").as_deref() {
                Err(_) | Ok("device") => true,
                Ok("host") => false,
                Ok(other) => panic!("KZ_HIP_DECODE must be device or host, got '{}'", other),
            },
            move_offsets: vec![],
            move_indices: vec![],
            n_sym: 0,
            sym_rng: None,
            sym_ids: vec![],
            average_symmetries: false,
            fell_back_boards: 0,
            audit,
            ranges: {
                // (a malformed value is not worth a panic in a constructor: no helpers, and say so once)
                let helpers: usize = match std::env::var("KZ_HIP_PREP_THREADS") {
                    Err(_) => 0,
                    Ok(v) => v.trim().parse().unwrap_or_else(|_| {
                        eprintln!("kz_hip: KZ_HIP_PREP_THREADS='{}' is not a number: using 0 helper threads", v);
                        0
                    }),
                }
                .min(8);
                (0..helpers + 1).map(|_| PrepRange::default()).collect()
            },
            sample_from: match StreamShift::from_env() {
                StreamShift::Auto(_) => Some(device),
                StreamShift::Fixed(_) => None,
            },
            ph: PhantomData,
        }
    }

    /// `RandomSymmetryNetwork::new(HipNetwork::new(..), rng, true)` (symmetry.rs:18-68) without its host work: every board
    /// of every batch gets a symmetry id drawn from `rng` at submit and the engine maps the planes on the way in and the
    /// policy indices on the way out, so this thread neither maps a board nor regenerates and searches its move list.
    /// Needs the decode on the device (the mapped logits never reach the host).
    pub fn new_with_symmetries(mapper: M, model: Arc<HipModel>, max_batch_size: usize, device: HipDevice, dtype: HipDtype, tables: &SymmetryTables, rng: Box<dyn rand::RngCore + Send>) -> Self {
        let mut net = Self::new(mapper, model, max_batch_size, device, dtype);
        assert!(net.device_decode, "random symmetries inside the launch need KZ_HIP_DECODE=device");
        let info = net._model.info;
        assert_eq!(tables.square_src.len(), tables.n_sym * (info.board_h * info.board_w) as usize);
        assert_eq!(tables.policy_map.len(), tables.n_sym * info.policy_len as usize);
        check(unsafe { kz_engine_set_symmetries(net.engine, tables.n_sym as c_int, tables.square_src.as_ptr(), tables.policy_map.as_ptr()) });
        net.n_sym = tables.n_sym;
        net.sym_rng = Some(rng);
        net
    }

    /// `AverageSymmetryNetwork::new(HipNetwork::new(..))` (symmetry.rs:70-124,150-184) without its host work: the engine
    /// evaluates every board under every row of `tables` and averages values and policy on the device
    /// (`kz_engine_submit_packed_decoded_avg`: the row order of the tables is the summation order).  This thread encodes
    /// each board once and receives one result per board.  `evaluate_batch` goes through the engine in chunks of
    /// `max_batch_size / n_sym` boards (the wrapper's `chunks(inner.max_batch_size())`, :108-113); `submit_batch` takes at
    /// most that many.  Exclusive with `new_with_symmetries`; needs the decode on the device.
    pub fn new_with_average_symmetries(mapper: M, model: Arc<HipModel>, max_batch_size: usize, device: HipDevice, dtype: HipDtype, tables: &SymmetryTables) -> Self {
        let mut net = Self::new(mapper, model, max_batch_size, device, dtype);
        assert!(net.device_decode, "averaged symmetries inside the engine need KZ_HIP_DECODE=device");
        let info = net._model.info;
        assert_eq!(tables.square_src.len(), tables.n_sym * (info.board_h * info.board_w) as usize);
        assert_eq!(tables.policy_map.len(), tables.n_sym * info.policy_len as usize);
        assert!(tables.n_sym >= 1 && tables.n_sym <= max_batch_size, "max_batch_size must hold one board under every symmetry");
        check(unsafe { kz_engine_set_symmetries(net.engine, tables.n_sym as c_int, tables.square_src.as_ptr(), tables.policy_map.as_ptr()) });
        net.n_sym = tables.n_sym;
        net.average_symmetries = true;
        net
    }

    /// The decoded submit of the batch `prepare` has staged: averaged over all symmetries, or with one drawn id per board
    /// (null ids without symmetries).
    fn submit_decoded(&mut self, slot: usize, bits_bytes: usize, n: usize) {
        if self.average_symmetries {
            assert!(n * self.n_sym <= self.max_batch_size, "an averaged batch is at most max_batch_size / n_sym boards");
            check(unsafe {
                kz_engine_submit_packed_decoded_avg(
                    self.engine,
                    slot as c_int,
                    self.bits.as_ptr(),
                    bits_bytes,
                    self.scalars_in.as_ptr(),
                    n as c_int,
                    self.move_offsets.as_ptr(),
                    self.move_indices.as_ptr(),
                )
            });
            return;
        }
        let sym = self.draw_symmetries(n);
        check(unsafe {
            kz_engine_submit_packed_decoded_sym(
                self.engine,
                slot as c_int,
                self.bits.as_ptr(),
                bits_bytes,
                self.scalars_in.as_ptr(),
                n as c_int,
                sym,
                self.move_offsets.as_ptr(),
                self.move_indices.as_ptr(),
            )
        });
    }

    /// One id per board of the batch being submitted (symmetry.rs:52); null without symmetries, which makes the `_sym`
    /// entries the plain ones (include/kz_hip.h).
    fn draw_symmetries(&mut self, n: usize) -> *const u8 {
        use rand::Rng;
        let n_sym = self.n_sym;
        match self.sym_rng.as_mut() {
            None => std::ptr::null(),
            Some(rng) => {
                self.sym_ids.clear();
                self.sym_ids.extend((0..n).map(|_| rng.gen_range(0..n_sym) as u8));
                self.sym_ids.as_ptr()
            }
        }
    }

    /// A batch's host work before the launch — `encode_input` of every board (cudnn.rs:61-64) and, with the decode on the
    /// device, the CSR move lists `move_offsets[b]..move_offsets[b + 1]` of `move_indices` — cut into contiguous ranges:
    /// this thread prepares the first, a scoped helper thread each of the others (a thread spawn is ~15 us against the
    /// ~250 us half a chess batch of 256 takes); the ranges meet in the staging vectors in board order.  Returns
    /// bits_bytes.  Same results as one thread doing it all.
    fn prepare(&mut self, boards: &[impl Borrow<B>], with_moves: bool) -> usize {
        let mapper = self.mapper;
        let bits_bytes = (mapper.input_bool_len() + 7) / 8;
        // (`impl Borrow<B>` says nothing about threads; `&B` is Send + Sync because `Board` is)
        let refs: Vec<&B> = boards.iter().map(|b| b.borrow()).collect();
        let n = refs.len();
        let parts = self.ranges.len().min((n / 16).max(1)); // a handful of boards: not worth a spawn
        let cut = |k: usize| n * k / parts;
        let (first, rest) = self.ranges.split_at_mut(1);
        let (bits_first, mut bits_rest) = self.bits[..n * bits_bytes].split_at_mut(cut(1) * bits_bytes);
        std::thread::scope(|scope| {
            for (k, range) in rest[..parts - 1].iter_mut().enumerate() {
                let (lo, hi) = (cut(k + 1), cut(k + 2));
                let (mine, tail) = std::mem::take(&mut bits_rest).split_at_mut((hi - lo) * bits_bytes);
                bits_rest = tail;
                let part = &refs[lo..hi];
                scope.spawn(move || prep_range(mapper, part, mine, with_moves, range));
            }
            prep_range(mapper, &refs[..cut(1)], bits_first, with_moves, &mut first[0]);
            // (the scope joins the helpers; a panic in one of them — `move_to_index` asserts — propagates here)
        });
        self.scalars_in.clear();
        self.move_offsets.clear();
        self.move_offsets.push(0);
        self.move_indices.clear();
        for range in &self.ranges[..parts] {
            self.scalars_in.extend_from_slice(&range.scalars);
            if with_moves {
                self.move_indices.extend_from_slice(&range.indices);
                for &c in &range.counts {
                    self.move_offsets.push(self.move_offsets.last().unwrap() + c);
                }
            }
        }
        assert_eq!(self.scalars_in.len(), n * mapper.input_scalar_count());
        if let Some(device) = self.sample_from {
            position_sample().offer(device, &self.bits, bits_bytes, &self.scalars_in, mapper.input_scalar_count(), n);
        }
        bits_bytes
    }

    /// `kz_engine_wait_decoded` through the status entry: the two views of the slot's pinned staging.  Boards the range
    /// fallback re-evaluated (status exactly `KZ_BOARD_FELL_BACK`: their results are the exact-f32 ones) are counted;
    /// any other non-zero status panics like the reference does on every executor error, naming the boards.
    fn wait_decoded_checked(&mut self, slot: usize, n: usize) -> (*const f32, *const f32) {
        let (mut values, mut probs) = (std::ptr::null::<f32>(), std::ptr::null::<f32>());
        let mut status = std::ptr::null_mut::<c_void>();
        check(unsafe { kz_engine_wait_decoded_status(self.engine, slot as c_int, &mut values, &mut probs, &mut status) });
        let status = unsafe { std::slice::from_raw_parts(status as *const u8, n) };
        self.fell_back_boards += status.iter().filter(|&&s| s == KZ_BOARD_FELL_BACK).count() as u64;
        let bad: Vec<usize> = (0..n).filter(|&b| status[b] != KZ_BOARD_OK && status[b] != KZ_BOARD_FELL_BACK).collect();
        if let Some(&first) = bad.first() {
            let what = if status[first] & KZ_BOARD_NONFINITE != 0 {
                "non-finite activation (beyond +-65504 the f16 and split-f16 paths overflow: set KZ_HIP_RANGE_FALLBACK=1 or KZ_HIP_DTYPE=f32)"
            } else {
                "Softmax input sum must be strictly positive (or a move index or symmetry id is out of range)"
            };
            panic!("kzhip: {} on boards {:?} of the batch", what, bad);
        }
        (values, probs)
    }

    /// values [n, 5] (tanh / softmax already applied on the device) + probabilities parallel to the move lists
    fn assemble(offsets: &[i64], values: &[f32], probs: &[f32]) -> Vec<ZeroEvaluation<'static>> {
        (0..offsets.len() - 1)
            .map(|bi| {
                let v = &values[bi * 5..bi * 5 + 5];
                let values = ZeroValuesPov {
                    value: ScalarPov::new(v[0]),
                    wdl: WDL { win: v[1], draw: v[2], loss: v[3] },
                    moves_left: v[4],
                };
                let policy = probs[offsets[bi] as usize..offsets[bi + 1] as usize].to_vec();
                ZeroEvaluation { values, policy: Cow::Owned(policy) }
            })
            .collect()
    }

    /// Asynchronous pair for `pipelined_executor_loop` (executor_pipelined.rs): encode, hand the batch to the engine
    /// and return while the GPU works.  At most `KZ_ENGINE_SLOTS` batches in flight.
    pub fn submit_batch(&mut self, boards: Vec<B>) {
        assert!(!boards.is_empty() && boards.len() <= self.max_batch_size);
        assert!(self.pending.len() < KZ_ENGINE_SLOTS, "every engine slot is in flight");
        let bits_bytes = self.prepare(&boards, self.device_decode);
        let slot = self.next_slot;
        if self.device_decode {
            self.submit_decoded(slot, bits_bytes, boards.len());
            // (the engine has copied the lists to its pinned staging: only the offsets are needed to cut up the reply)
            self.pending.push_back((slot, vec![], self.move_offsets.clone()));
        } else {
            check(unsafe {
                kz_engine_submit_packed(
                    self.engine,
                    slot as c_int,
                    self.bits.as_ptr(),
                    bits_bytes,
                    self.scalars_in.as_ptr(),
                    boards.len() as c_int,
                )
            });
            self.pending.push_back((slot, boards, vec![]));
        }
        self.next_slot = (slot + 1) % KZ_ENGINE_SLOTS;
    }

    /// Results of the OLDEST submitted batch.
    pub fn wait_batch(&mut self) -> Vec<ZeroEvaluation<'static>> {
        let (slot, boards, offsets) = self.pending.pop_front().expect("wait_batch with nothing in flight");
        if self.device_decode {
            let (n, total) = (offsets.len() - 1, *offsets.last().unwrap() as usize);
            let (values, probs) = self.wait_decoded_checked(slot, n);
            // views into the engine's pinned staging, valid until the next submit on this slot (include/kz_hip.h)
            let values = unsafe { std::slice::from_raw_parts(values, n * 5) };
            let probs = if total == 0 { &[][..] } else { unsafe { std::slice::from_raw_parts(probs, total) } };
            return Self::assemble(&offsets, values, probs);
        }
        // decode straight from the engine's pinned staging (no copy of the 1.9 MB policy tensor into a Vec first)
        let (mut scalars, mut policy) = (std::ptr::null::<f32>(), std::ptr::null::<f32>());
        check(unsafe { kz_engine_wait_view(self.engine, slot as c_int, &mut scalars, &mut policy) });
        let (batch_size, policy_len) = (boards.len(), self.mapper.policy_len());
        let outputs = unsafe {
            [std::slice::from_raw_parts(scalars, batch_size * 5), std::slice::from_raw_parts(policy, batch_size * policy_len)]
        };
        decode_output(self.mapper, &boards, &outputs)
    }
}

impl<B: Board, M: BoardMapper<B>> Drop for HipNetwork<B, M> {
    fn drop(&mut self) {
        if self.audit {
            // one line per network generation: what the sampled boards deviated by from the <= 1e-4 arithmetic
            let mut st = KzAuditStats::default();
            if unsafe { kz_engine_audit_stats(self.engine, &mut st as *mut KzAuditStats as *mut c_void, 0) } == 0 {
                let rms = |sum_sq: f64, n: i64| if n > 0 { (sum_sq / n as f64).sqrt() } else { 0.0 };
                eprintln!(
                    "kz_hip audit: batches {} boards {} moves {} skipped {} | max|dp| {:.3e} rms dp {:.3e} | max|d| value {:.3e} wdl {:.3e} moves_left {:.3e}",
                    st.batches, st.boards, st.moves, st.skipped, st.max_abs_prob, rms(st.sum_sq_prob, st.moves), st.max_abs_value[0],
                    st.max_abs_value[1].max(st.max_abs_value[2]).max(st.max_abs_value[3]), st.max_abs_value[4]
                );
            }
        }
        unsafe { kz_engine_destroy(self.engine) }
    }
}

impl<B: Board, M: BoardMapper<B>> Network<B> for HipNetwork<B, M> {
    fn max_batch_size(&self) -> usize {
        self.max_batch_size
    }

    fn evaluate_batch(&mut self, boards: &[impl Borrow<B>]) -> Vec<ZeroEvaluation<'static>> {
        let batch_size = boards.len();
        assert!(batch_size <= self.max_batch_size);
        if batch_size == 0 {
            return vec![];
        }

        assert!(self.pending.is_empty(), "evaluate_batch while submitted batches are in flight");
        if self.average_symmetries && batch_size * self.n_sym > self.max_batch_size {
            // the engine takes max_batch_size / n_sym boards per averaged call: chunk like the wrapper (symmetry.rs:108-113)
            let chunk = self.max_batch_size / self.n_sym;
            return boards.chunks(chunk).flat_map(|part| self.evaluate_batch(part)).collect();
        }
        let bits_bytes = self.prepare(boards, self.device_decode);

        if self.device_decode {
            self.submit_decoded(0, bits_bytes, batch_size);
            let (values, probs) = self.wait_decoded_checked(0, batch_size);
            let total = *self.move_offsets.last().unwrap() as usize;
            let values = unsafe { std::slice::from_raw_parts(values, batch_size * 5) };
            let probs = if total == 0 { &[][..] } else { unsafe { std::slice::from_raw_parts(probs, total) } };
            return Self::assemble(&self.move_offsets, values, probs);
        }

        check(unsafe {
            kz_engine_eval_packed(
                self.engine,
                self.bits.as_ptr(),
                bits_bytes,
                self.scalars_in.as_ptr(),
                batch_size as c_int,
                self.scalars_out.as_mut_ptr(),
                self.policy_out.as_mut_ptr(),
            )
        });

        let policy_len = self.mapper.policy_len();
        let outputs = [&self.scalars_out[..batch_size * 5], &self.policy_out[..batch_size * policy_len]];
        decode_output(self.mapper, boards, &outputs)
    }
}

impl<B: Board, M: BoardMapper<B>> Debug for HipNetwork<B, M> {
    fn fmt(&self, f: &mut Formatter<'_>) -> std::fmt::Result {
        f.debug_struct("HipNetwork")
            .field("mapper", &self.mapper)
            .field("max_batch_size", &self.max_batch_size)
            .finish()
    }
}
