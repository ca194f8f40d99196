"""kz_model_range_profile_fast on the GPU: the range profile taken inside the one-launch exact-f32 tower (the PROFILE instances of
kz_tower_resident_f32, kz_tower_f32.hip), held to the oracle's trace and to kz_model_range_profile, the per-layer entry.

Shapes, the smallest at which the kernel can go wrong — one per instance and corner, every network depth 2:
  ataxx7x128  Ataxx 7x7 ataxx_conv   <128, 7>: two boards per workgroup, a board boundary inside tile 3, 14 padding rows to ignore
  ttt128      ttt 3x3 dense          <128, 7>: twelve boards per workgroup, up to three boards in one tile of 16 rows
  chess256    chess attention, Q 64  <256, 4>: one board per workgroup
  chess128    chess attention, Q 64  <128, 4>
  go9x128     Go 9x9 conv            <128, 6>: 81 of 96 rows
  go19x64     Go 19x19 2x64          no one-launch tower: the call IS the per-layer profile
Batches 1, 13 and 259: 259 is odd — the last workgroup of the two-board instance holds one board — and crosses the internal
engine's chunk of 256.  The thirteen boards are cycled from the fourth, as in tests/test_gpu_range_profile.py.

1. Exact networks (tests/exact_nets.py; draw_exact keeps a seed only if conditions_hold): `==` with the oracle's maxima and with
   kz_model_range_profile; every site alive.
2. Random networks: within the project's f32 bound 1e-4 * max(1, value) of the oracle's trace (tests/test_gpu_parity.py).
3. Invariance, `==`: the profile of a subset is the subset of the profile; a board's value does not depend on its place in the
   batch, its workgroup partners or the side of the chunk boundary it falls on.
4. The scaled network of tests/test_gpu_bf16.py (stream times 2^12): shifted sites exactly 4096 x, the last site equal.
5. Non-finite rule on the two-boards-per-workgroup shape: the bad board +inf at every site, its workgroup partner and all others `==`.
6. Go 19x19: path conv_igemm_f32, outputs `==` the existing entry's.
7. The refusals, in this function's name.
8. An ordinary exact-f32 engine of a profiled model (it shares the cached weight stream) returns the bits it returned before.
"""
import numpy as np
import pytest

from kzero_amd import capi, synth
from kzero_amd.model_file import write_model
from tests import exact_nets as E
from tests import oracle_lib as O
from tests.test_gpu_range_profile import scaled_stream

pytestmark = pytest.mark.gpu

F32_ATOL = 1e-4  # the project's f32 bound (tests/test_gpu_parity.py): 1e-4 * max(1, value)
BOARDS = 13
BATCHES = (1, 13, 259)
CHUNK = 256  # the internal engine's max_batch on the one-launch path

# (id, game, channels, head, range_profile_fast_path, plan(256, f32)[0])
SHAPES = [
    ("ataxx7x128", "ataxx-7", 128, "ataxx_conv", "tower_resident_f32", "tower_resident_f32+heads"),
    ("ttt128", "ttt", 128, "dense", "tower_resident_f32", "tower_resident_f32"),
    ("chess256", "chess", 256, "attention", "tower_resident_f32", "tower_resident_f32"),
    ("chess128", "chess", 128, "attention", "tower_resident_f32", "tower_resident_f32"),
    ("go9x128", "go-9", 128, "conv", "tower_resident_f32", "tower_resident_f32+heads"),
    ("go19x64", "go-19", 64, "conv", "conv_igemm_f32", "conv_igemm_f32"),
]
NAMES = [s[0] for s in SHAPES]
RESIDENT = [s[0] for s in SHAPES if s[4] == "tower_resident_f32"]


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


class Ref:
    """A network, its thirteen boards and the oracle's trace: per site the maximum of |x| per board.  Computed once per module
    (the pattern of tests/test_gpu_range_profile.py)."""
    _cache = {}

    def __init__(self, shape, blob, bits, scalars_in):
        self.blob, self.bits, self.scalars_in = blob, bits, scalars_in
        net = O.OracleNet(blob)
        x = O.encode_input_full(bits, scalars_in, net.n_scalar, net.n_bool, net.h, net.w)
        _, _, acts = net.forward_trace(x)
        self.model = capi.Model(blob=blob)
        # a shape that silently takes another instance fails here instead of weakening the test
        assert self.model.range_profile_fast_path() == shape[4], (shape[0], self.model.range_profile_fast_path())
        assert self.model.plan(256, capi.KZ_DTYPE_F32)[0] == shape[5], (shape[0], self.model.plan(256, capi.KZ_DTYPE_F32))
        self.sites = self.model.range_sites()
        assert len(self.sites) == 2 * net.depth + 1 and f"tower.{net.depth}" not in self.sites
        n = bits.shape[0]
        self.per_board = np.stack([np.abs(acts[s]).reshape(n, -1).max(axis=1) for s in self.sites]).astype(np.float32)
        for a in (self.bits, self.scalars_in, self.per_board):
            a.setflags(write=False)

    def expect(self, idx):
        """(site maxima, board maxima over the shifted sites) of the boards idx."""
        pb = self.per_board[:, idx]
        return pb.max(axis=1), pb[:-1].max(axis=0)

    @classmethod
    def get(cls, name, kind):
        if (name, kind) not in cls._cache:
            shape = next(s for s in SHAPES if s[0] == name)
            _, game, channels, head = shape[:4]
            kw = dict(query_channels=64) if head == "attention" else {}
            if kind == "exact":
                bits, scalars_in = E.exact_boards(game, BOARDS, E.SEED)
                # (draw_exact redraws the seed until conditions_hold: only such a network comes back)
                meta, tensors, _, out = E.draw_exact(game, 2, channels, head, None, E.SEED, boards=(bits, scalars_in), **kw)
                assert E.conditions_hold(out[2])
                blob = write_model(meta, tensors)
            else:
                bits, scalars_in = synth.random_boards(game, BOARDS, seed=3)
                blob = synth.random_model(game, 2, channels, head, seed=5, **kw)
            cls._cache[name, kind] = cls(shape, blob, bits, scalars_in)
        return cls._cache[name, kind]


def pick(batch):
    """`batch` of the thirteen boards, starting at the fourth so that no chunk starts the cycle."""
    return (np.arange(batch) + 3) % BOARDS


# ---- 1. exact networks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", NAMES)
def test_exact_networks_report_the_oracle_maxima(dev, name, batch):
    r = Ref.get(name, "exact")
    idx = pick(batch)
    site_max, board_max = r.model.range_profile_fast(dev, r.bits[idx], r.scalars_in[idx])
    want_sites, want_boards = r.expect(idx)
    print(f"[range fast] {name} exact, {batch} boards: " + ", ".join(f"{s} {v:g}" for s, v in zip(r.sites, site_max)))
    assert want_sites.min() > 0 and site_max.min() > 0  # (every site is alive)
    assert site_max.dtype == np.float32 and site_max.shape == (len(r.sites),) and board_max.shape == (batch,)
    assert np.array_equal(site_max, want_sites), (site_max, want_sites)
    assert np.array_equal(board_max, want_boards), np.flatnonzero(board_max != want_boards)
    slow_sites, slow_boards = r.model.range_profile(dev, r.bits[idx], r.scalars_in[idx])
    assert np.array_equal(site_max, slow_sites) and np.array_equal(board_max, slow_boards)


# ---- 2. random networks, 3. invariance ------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", NAMES)
def test_random_networks_within_the_f32_bound(dev, name, batch):
    r = Ref.get(name, "random")
    idx = pick(batch)
    site_max, board_max = r.model.range_profile_fast(dev, r.bits[idx], r.scalars_in[idx])
    want_sites, want_boards = r.expect(idx)
    d_sites = np.abs(site_max - want_sites) / np.maximum(1.0, want_sites)
    d_boards = np.abs(board_max - want_boards) / np.maximum(1.0, want_boards)
    print(f"[range fast] {name} random, {batch} boards: max |d| / max(1, value) = {max(d_sites.max(), d_boards.max()):.3e}")
    assert d_sites.max() <= F32_ATOL and d_boards.max() <= F32_ATOL


@pytest.mark.parametrize("name", NAMES)
def test_a_board_reports_the_same_wherever_it_stands(dev, name):
    r = Ref.get(name, "random")
    idx = pick(259)
    site_max, board_max = r.model.range_profile_fast(dev, r.bits[idx], r.scalars_in[idx])
    # the same thirteen boards again and again: 13 is odd, so a board changes its slot in the workgroup and its partners from
    # one cycle to the next, and the cycles behind board 256 run in the second chunk
    cycle = board_max[:BOARDS]
    for lo in range(BOARDS, 259, BOARDS):
        n = min(BOARDS, 259 - lo)
        assert np.array_equal(board_max[lo:lo + n], cycle[:n]), lo
    assert lo + n == 259 and lo < CHUNK < 259
    # the profile of a subset is the subset of the profile: a head, a tail that starts at an odd place, single boards
    for sub in (slice(0, 5), slice(7, 12), slice(258, 259), slice(4, 5)):
        sites_sub, boards_sub = r.model.range_profile_fast(dev, r.bits[idx[sub]], r.scalars_in[idx[sub]])
        assert np.array_equal(boards_sub, board_max[sub]), sub
        assert np.array_equal(sites_sub, r.model.range_profile_fast(dev, r.bits[idx[sub]][::-1], r.scalars_in[idx[sub]][::-1])[0])
    # beside another partner: the boards in reverse order report the reverse
    _, reversed_boards = r.model.range_profile_fast(dev, r.bits[idx[:BOARDS]][::-1], r.scalars_in[idx[:BOARDS]][::-1])
    assert np.array_equal(reversed_boards[::-1], cycle)
    assert np.array_equal(site_max[:-1].max(), board_max.max())


# ---- 4. the scaled network ------------------------------------------------------------------------------------------------
S = 2.0 ** 12


def test_scaled_network_is_4096_times_the_original(dev):
    blob = synth.random_model("chess", 2, 256, "attention", seed=5, block_gain=64.0)
    bits, scalars_in = synth.random_boards("chess", 37, seed=3)
    model, scaled = capi.Model(blob=blob), capi.Model(blob=scaled_stream(blob))
    assert model.range_profile_fast_path() == scaled.range_profile_fast_path() == "tower_resident_f32"
    site, board = model.range_profile_fast(dev, bits, scalars_in)
    site_s, board_s = scaled.range_profile_fast(dev, bits, scalars_in)
    print(f"[range fast] chess 2x256, stream x 2^12: sites {site_s.tolist()}, boards {board_s.min():.0f} .. {board_s.max():.0f}")
    assert np.array_equal(site_s[:-1], site[:-1] * np.float32(S))
    assert site_s[-1] == site[-1]
    assert np.array_equal(board_s, board * np.float32(S))
    assert (board_s > 65504.0).all()


# ---- 5. non-finite inputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad_value", [np.inf, -np.inf, np.nan])
def test_a_non_finite_board_reports_inf_and_touches_no_other(dev, bad_value):
    r = Ref.get("ataxx7x128", "random")  # two boards per workgroup: board 5 shares its workgroup with board 4
    bad, partner = 5, 4
    scalars_in = r.scalars_in.copy()
    scalars_in[bad, 0] = bad_value
    clean_sites, clean_boards = r.model.range_profile_fast(dev, r.bits, r.scalars_in)
    site_max, board_max = r.model.range_profile_fast(dev, r.bits, scalars_in)
    assert (site_max == np.inf).all(), site_max  # +inf, never NaN
    assert board_max[bad] == np.inf
    assert board_max[partner] == clean_boards[partner]
    others = np.arange(BOARDS) != bad
    assert np.array_equal(board_max[others], clean_boards[others])
    # that board alone: +inf at every site; the partner alone with it: its own maxima at every site
    alone, _ = r.model.range_profile_fast(dev, r.bits[bad:bad + 1], scalars_in[bad:bad + 1])
    assert alone.shape == clean_sites.shape and (alone == np.inf).all(), alone
    partner_sites, _ = r.model.range_profile_fast(dev, r.bits[partner:partner + 1], r.scalars_in[partner:partner + 1])
    rest_sites, rest_boards = r.model.range_profile_fast(dev, r.bits[others], scalars_in[others])
    assert np.isfinite(rest_sites).all() and np.array_equal(rest_boards, clean_boards[others])
    assert (rest_sites >= partner_sites).all()
    want_sites, want_boards = r.expect(np.flatnonzero(others))
    assert (np.abs(rest_sites - want_sites) <= F32_ATOL * np.maximum(1.0, want_sites)).all()
    assert (np.abs(rest_boards - want_boards) <= F32_ATOL * np.maximum(1.0, want_boards)).all()


# ---- 6. no one-launch tower -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", (13, 69))
def test_go19_is_the_per_layer_profile(dev, batch):
    r = Ref.get("go19x64", "random")
    assert r.model.range_profile_fast_path() == "conv_igemm_f32"
    idx = pick(batch)
    fast = r.model.range_profile_fast(dev, r.bits[idx], r.scalars_in[idx])
    slow = r.model.range_profile(dev, r.bits[idx], r.scalars_in[idx])
    assert np.array_equal(fast[0], slow[0]) and np.array_equal(fast[1], slow[1])


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_carry_this_functions_name(dev):
    lib = capi.load()
    bits, scalars = np.zeros((1, 512), np.uint8), np.zeros((1, 16), np.float32)
    out = np.zeros(64, np.float32)
    buf = capi.C.create_string_buffer(32)

    def profile(model, batch=1, stride=512):
        assert lib.kz_model_range_profile_fast(model._h, dev, bits.ctypes.data, stride, scalars.ctypes.data, batch, out.ctypes.data, None) != 0
        return lib.kz_last_error().decode()

    def path(model, length=32):
        assert lib.kz_model_range_profile_fast_path(model._h, buf, length) != 0
        return lib.kz_last_error().decode()

    attention = capi.Model(blob=O.load_blob("chess_att2x64"))
    dense = capi.Model(blob=O.load_blob("sttt_dn1x64"))
    stem_only = capi.Model(blob=synth.random_model("chess", 0, 64, "attention", seed=1))
    for model, needle in ((attention, "ResTower"), (dense, "ResTower"), (stem_only, "without blocks")):
        assert profile(model).startswith("kz_model_range_profile_fast: ") and needle in profile(model), profile(model)
        assert path(model).startswith("kz_model_range_profile_fast_path: ") and needle in path(model), path(model)
    res = Ref.get("ataxx7x128", "random").model
    assert profile(res, batch=0) == "kz_model_range_profile_fast: batch must be positive"
    assert profile(res, stride=3) == "kz_model_range_profile_fast: bits_stride too small"
    assert "buffer" in path(res, 8)
    assert not any("KZ_" in m for m in (profile(attention), profile(stem_only), path(res, 8)))


# ---- 8. the shared weight stream ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ataxx7x128", "chess256"])
def test_a_profiled_model_still_plans_and_runs_as_before(dev, name):
    """The internal engine is the one-launch f32 tower without heads on the model's cached weight stream: an ordinary exact-f32
    engine alive across the profile — with the heads inside (Ataxx) or behind (chess) — returns the same bits afterwards, and so
    does one created after it."""
    r = Ref.get(name, "random")
    want = next(s for s in SHAPES if s[0] == name)[5]
    eng = capi.Engine(r.model, dev, 64, capi.KZ_DTYPE_F32)
    assert eng.tower_path == want
    before = eng.eval_packed(r.bits, r.scalars_in)
    site_max, _ = r.model.range_profile_fast(dev, r.bits, r.scalars_in)
    assert np.isfinite(site_max).all() and site_max.min() > 0
    after = eng.eval_packed(r.bits, r.scalars_in)
    assert eng.tower_path == want
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    fresh = capi.Engine(r.model, dev, 64, capi.KZ_DTYPE_F32).eval_packed(r.bits, r.scalars_in)
    assert np.array_equal(before[0], fresh[0]) and np.array_equal(before[1], fresh[1])
