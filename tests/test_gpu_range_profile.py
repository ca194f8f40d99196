"""kz_model_range_profile on the GPU: max |x| of every tensor an f16 / split16 tower kernel stores, measured in exact f32 by
kz_range_absmax (kz_range_profile.hip) behind the per-layer implicit GEMM.

1. Exact networks (tests/exact_nets.py, narrow family, depth 2): every site maximum == the maximum of |OracleNet.forward_trace| of
   that site, and every board's maximum == the oracle's over the sites a shift moves.  max is order-independent and the networks
   are exact in f32, so this is `==`.
2. Random networks of the same shapes: within the project's f32 bound, 1e-4 * max(1, value).
   Shapes, the smallest at which the kernel can go wrong: Ataxx 7x7 2x16 (49 squares, 16 channels inside 32-wide rows: half of
   every row is padding the kernel must not read as data), chess 2x64, Go 9x9 (7 bool planes) 2x48 (channels no multiple of 32),
   Go 19x19 2x64 (361 squares: more than one pass of the 256 threads).  Batches 13, 1 and 69: 69 crosses the internal engine's
   chunk of 64.
3. The scaled network of tests/test_gpu_bf16.py (stream times 2^12, the same function): its shifted sites are exactly 4096 x the
   original's, its last site is the original's, every board is past 65504.
4. Non-finite rule: a board with an infinite scalar plane reports +inf at every site; the other boards' maxima do not change.
"""
import numpy as np
import pytest

from kzero_amd import capi, synth
from kzero_amd.model_file import read_model, write_model
from tests import exact_nets as E
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

F32_ATOL = 1e-4  # the project's f32 bound (tests/test_gpu_parity.py): 1e-4 * max(1, value)
BOARDS = 13
BATCHES = (13, 1, 69)

# (id, game, channels, head)
SHAPES = [
    ("ataxx7x16", "ataxx-7", 16, "ataxx_conv"),
    ("chess64", "chess", 64, "attention"),
    ("go9x48", "go-9", 48, "conv"),
    ("go19x64", "go-19", 64, "conv"),
]


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


class Ref:
    """A network, its thirteen boards and the oracle's trace: per site the maximum of |x| per board.  Computed once per module."""
    _cache = {}

    def __init__(self, blob, bits, scalars_in):
        self.blob, self.bits, self.scalars_in = blob, bits, scalars_in
        net = O.OracleNet(blob)
        x = O.encode_input_full(bits, scalars_in, net.n_scalar, net.n_bool, net.h, net.w)
        _, _, acts = net.forward_trace(x)
        self.model = capi.Model(blob=blob)
        self.sites = self.model.range_sites()
        assert len(self.sites) == 2 * net.depth + 1 and f"tower.{net.depth}" not in self.sites
        n = bits.shape[0]
        # [site][board], f32 like the tensors themselves
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
            _, game, channels, head = next(s for s in SHAPES if s[0] == name)
            kw = dict(query_channels=64) if head == "attention" else {}
            if kind == "exact":
                bits, scalars_in = E.exact_boards(game, BOARDS, E.SEED)
                meta, tensors, _, _ = E.draw_exact(game, 2, channels, head, None, E.SEED, boards=(bits, scalars_in), **kw)
                blob = write_model(meta, tensors)
            else:
                bits, scalars_in = synth.random_boards(game, BOARDS, seed=3)
                blob = synth.random_model(game, 2, channels, head, seed=5, **kw)
            cls._cache[name, kind] = cls(blob, bits, scalars_in)
        return cls._cache[name, kind]


def pick(batch):
    """`batch` of the thirteen boards, starting at the fourth so that no chunk starts the cycle."""
    return (np.arange(batch) + 3) % BOARDS


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_exact_networks_report_the_oracle_maxima(dev, name, batch):
    r = Ref.get(name, "exact")
    idx = pick(batch)
    site_max, board_max = r.model.range_profile(dev, r.bits[idx], r.scalars_in[idx])
    want_sites, want_boards = r.expect(idx)
    print(f"[range] {name} exact, {batch} boards: " + ", ".join(f"{s} {v:g}" for s, v in zip(r.sites, site_max)))
    assert want_sites.min() > 0  # (every site is alive)
    assert site_max.dtype == np.float32 and site_max.shape == (len(r.sites),) and board_max.shape == (batch,)
    assert np.array_equal(site_max, want_sites), (site_max, want_sites)
    assert np.array_equal(board_max, want_boards), np.flatnonzero(board_max != want_boards)


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_random_networks_within_the_f32_bound(dev, name, batch):
    r = Ref.get(name, "random")
    idx = pick(batch)
    site_max, board_max = r.model.range_profile(dev, r.bits[idx], r.scalars_in[idx])
    want_sites, want_boards = r.expect(idx)
    d_sites = np.abs(site_max - want_sites) / np.maximum(1.0, want_sites)
    d_boards = np.abs(board_max - want_boards) / np.maximum(1.0, want_boards)
    print(f"[range] {name} random, {batch} boards: max |d| / max(1, value) = {max(d_sites.max(), d_boards.max()):.3e}")
    assert d_sites.max() <= F32_ATOL and d_boards.max() <= F32_ATOL
    # the profile of a subset is the subset of the profile: nothing depends on the batch or its split into chunks
    if batch == 69:
        _, first = r.model.range_profile(dev, r.bits[idx[:5]], r.scalars_in[idx[:5]])
        assert np.array_equal(first, board_max[:5])
        assert np.array_equal(board_max[:BOARDS], board_max[BOARDS:2 * BOARDS])  # (the same boards again, in the next places)
        assert np.array_equal(board_max[64:], board_max[64 - 4 * BOARDS:69 - 4 * BOARDS])  # (and behind the chunk boundary)


def test_a_profiled_model_still_plans_and_runs_as_before(dev):
    """The internal engine takes the per-layer path whatever the plan says, and leaves nothing behind: the model's own f32 engine
    is the one-launch tower before and after, and gives the same bits."""
    model = capi.Model(blob=synth.random_model("ataxx-7", 2, 128, "ataxx_conv", seed=5))
    bits, scalars_in = synth.random_boards("ataxx-7", 9, seed=3)
    assert model.plan(64, capi.KZ_DTYPE_F32)[0] == "tower_resident_f32+heads"
    eng = capi.Engine(model, dev, 64, capi.KZ_DTYPE_F32)
    before = eng.eval_packed(bits, scalars_in)
    site_max, _ = model.range_profile(dev, bits, scalars_in)
    assert np.isfinite(site_max).all() and site_max.min() > 0
    after = eng.eval_packed(bits, scalars_in)
    assert eng.tower_path == "tower_resident_f32+heads"
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


# ---- 3. the scaled network ------------------------------------------------------------------------------------------------
S = 2.0 ** 12


def scaled_stream(blob):
    """tests/test_gpu_bf16.py's recipe.  The same function with the residual stream S times as large: the stem's weights and
    bias times S, every block's (folded) bias times S, the final BN's running mean times S and its variance times S^2.  bn_eps is
    one number for the whole network, so it goes up by S^2 with the final BN's variance — and every block BatchNorm takes the
    scaling that keeps its fold (conv bias - mean) * k + beta, k = gamma / sqrt(var + eps), the same function of an S times larger
    input: conv bias, mean and beta times S (the folded bias times S), var times S^2 and gamma times S (k unchanged).  Powers of
    two throughout: the oracle returns the unscaled network's bits."""
    meta, t = read_model(blob)
    t = {k: v.copy() for k, v in t.items()}
    depth, s1, s2 = meta["tower_depth"], np.float32(S), np.float32(S * S)
    t["common.tower.0.weight"] *= s1
    t["common.tower.0.bias"] *= s1
    for i in range(1, depth + 1):
        for conv, bn in ((0, 1), (3, 4)):
            t[f"common.tower.{i}.seq.{conv}.bias"] *= s1
            for n in ("weight", "bias", "running_mean"):
                t[f"common.tower.{i}.seq.{bn}.{n}"] *= s1
            t[f"common.tower.{i}.seq.{bn}.running_var"] *= s2
    t[f"common.tower.{depth + 1}.running_mean"] *= s1
    t[f"common.tower.{depth + 1}.running_var"] *= s2
    meta = dict(meta)
    meta["bn_eps"] = float(np.float32(meta["bn_eps"]) * s2)
    return write_model(meta, t)


def test_scaled_network_is_4096_times_the_original(dev):
    blob = synth.random_model("chess", 2, 256, "attention", seed=5, block_gain=64.0)
    bits, scalars_in = synth.random_boards("chess", 37, seed=3)
    site, board = capi.Model(blob=blob).range_profile(dev, bits, scalars_in)
    site_s, board_s = capi.Model(blob=scaled_stream(blob)).range_profile(dev, bits, scalars_in)
    print(f"[range] chess 2x256, stream x 2^12: sites {site_s.tolist()}, boards {board_s.min():.0f} .. {board_s.max():.0f}")
    assert np.array_equal(site_s[:-1], site[:-1] * np.float32(S))
    assert site_s[-1] == site[-1]
    assert np.array_equal(board_s, board * np.float32(S))
    assert (board_s > 65504.0).all()
    # and the shift takes it back: the profile of shift(scaled, 12) is the original's
    site_b, board_b = capi.Model(blob=scaled_stream(blob)).stream_shift(12).range_profile(dev, bits, scalars_in)
    assert np.array_equal(site_b, site) and np.array_equal(board_b, board)


# ---- 4. non-finite inputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad_value", [np.inf, -np.inf, np.nan])
def test_a_non_finite_board_reports_inf_and_touches_no_other(dev, bad_value):
    r = Ref.get("ataxx7x16", "random")
    bad = 5
    scalars_in = r.scalars_in.copy()
    scalars_in[bad, 0] = bad_value
    clean_sites, clean_boards = r.model.range_profile(dev, r.bits, r.scalars_in)
    site_max, board_max = r.model.range_profile(dev, r.bits, scalars_in)
    assert (site_max == np.inf).all(), site_max  # +inf, never NaN
    assert board_max[bad] == np.inf
    others = np.arange(BOARDS) != bad
    assert np.array_equal(board_max[others], clean_boards[others])
    # that board alone: +inf at every site; the others alone: their own maxima, as without it
    alone, _ = r.model.range_profile(dev, r.bits[bad:bad + 1], scalars_in[bad:bad + 1])
    assert alone.shape == clean_sites.shape and (alone == np.inf).all(), alone
    rest_sites, rest_boards = r.model.range_profile(dev, r.bits[others], scalars_in[others])
    want_sites, want_boards = r.expect(np.flatnonzero(others))
    assert np.isfinite(rest_sites).all() and np.array_equal(rest_boards, clean_boards[others])
    assert (np.abs(rest_sites - want_sites) <= F32_ATOL * np.maximum(1.0, want_sites)).all()
    assert (np.abs(rest_boards - want_boards) <= F32_ATOL * np.maximum(1.0, want_boards)).all()
