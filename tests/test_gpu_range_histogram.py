"""kz_model_range_histogram and kz_model_range_histogram_fast on the GPU: the binade counts of every stored tower tensor, taken
per layer (kz_range_histogram, kz_range_profile.hip) and inside the one-launch exact-f32 tower (the histogram instances of
kz_tower_resident_f32, kz_tower_f32.hip), held to the oracle's trace binned by tests/range_hist_ref.py.

The six depth-2 shapes, the batches 1, 13 and 259 and the thirteen boards cycled from the fourth are those of
tests/test_gpu_range_profile_fast.py (its SHAPES say which instance a shape takes and what it covers); each shape asserts
range_profile_fast_path and plan(256, f32)[0] as there.

1. Exact networks: fast == per layer == the oracle's bins, `==`; every site has zeros and at least two binades; rows sum to
   batch * hw * C.
2. The far bins: the exact networks through stream_shift with k = 24, -24 and 24 three times (the bottom end bin): the shifted
   sites' histograms are the original's moved by k bins with the ends absorbing, the last site identical, `==`.
3. Additivity on random networks, `==`: 259 boards = the first 100 + the rest; the boards reversed; 259 cycled boards = the
   integer combination of single-board histograms the cycle implies.
4. Random networks against the oracle: per site sum_b |gpu - oracle| <= 2 A, A = the elements within 1e-4 * max(1, |x|) of a binade
   boundary plus twice the non-zero elements with |x| <= 1e-4, A <= 1 % of the site asserted; the totals exact.
5. Non-finite values on the two-boards-per-workgroup shape.
6. Go 19x19 takes the per-layer path.
7. Refusals in each function's name.
8. Ordinary engines, and range_profile_fast, return what they returned before a histogram call.
"""
import numpy as np
import pytest

from kzero_amd import capi, synth
from kzero_amd.model_file import write_model
from tests import exact_nets as E
from tests import oracle_lib as O
from tests import range_hist_ref as R
from tests.test_gpu_range_profile_fast import BATCHES, BOARDS, CHUNK, NAMES, SHAPES, pick

pytestmark = pytest.mark.gpu

F32_ATOL = 1e-4  # the project's f32 bound (tests/test_gpu_parity.py): 1e-4 * max(1, value)


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


class Ref:
    """A network, its thirteen boards and the oracle's trace: per site and board the 96 counts (and the trace itself, for
    the bound of the random networks).  Computed once per module."""
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
        assert len(self.sites) == 2 * net.depth + 1
        n = bits.shape[0]
        self.per_board_elems = net.h * net.w * net.channels
        self.trace = [np.asarray(acts[s], np.float32).reshape(n, -1) for s in self.sites]
        assert all(t.shape[1] == self.per_board_elems for t in self.trace)
        self.per_board = np.stack([np.stack([R.histogram_of(t[b]) for b in range(n)]) for t in self.trace])  # [site, board, 96]
        for a in (self.bits, self.scalars_in, self.per_board, *self.trace):
            a.setflags(write=False)

    def near(self):
        """near_a_boundary per site and board, [site, board] (the random networks' bound)."""
        if not hasattr(self, "_near"):
            self._near = np.array([[near_a_boundary(t[b]) for b in range(t.shape[0])] for t in self.trace])
        return self._near

    def expect(self, idx):
        """uint64 [n_sites, 96] of the boards idx (with repetitions)."""
        return self.per_board[:, idx].sum(axis=1, dtype=np.uint64)

    def hist(self, dev, idx, fast=True, scalars_in=None):
        s = self.scalars_in if scalars_in is None else scalars_in
        h = self.model.range_histogram(dev, self.bits[idx], s[idx], fast=fast)
        assert h.dtype == np.uint64 and h.shape == (len(self.sites), capi.KZ_RANGE_BINS)
        # every element of every real board and channel is counted once, whatever else is wrong
        assert (h.sum(axis=1) == len(idx) * self.per_board_elems).all(), (h.sum(axis=1), len(idx) * self.per_board_elems)
        return h

    @classmethod
    def get(cls, name, kind):
        if (name, kind) not in cls._cache:
            shape = next(s for s in SHAPES if s[0] == name)
            _, game, channels, head = shape[:4]
            kw = dict(query_channels=64) if head == "attention" else {}
            if kind == "exact":
                bits, scalars_in = E.exact_boards(game, BOARDS, E.SEED)
                meta, tensors, _, out = E.draw_exact(game, 2, channels, head, None, E.SEED, boards=(bits, scalars_in), **kw)
                assert E.conditions_hold(out[2])
                blob = write_model(meta, tensors)
            else:
                bits, scalars_in = synth.random_boards(game, BOARDS, seed=3)
                blob = synth.random_model(game, 2, channels, head, seed=5, **kw)
            cls._cache[name, kind] = cls(shape, blob, bits, scalars_in)
        return cls._cache[name, kind]


def show(tag, sites, h):
    for s, row in zip(sites, h):
        nz = np.flatnonzero(row)
        print(f"[range hist] {tag} {s}: " + " ".join(f"{b}:{int(row[b])}" for b in nz))


# ---- 1. exact networks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", NAMES)
def test_exact_networks_count_the_oracle_bins(dev, name, batch):
    r = Ref.get(name, "exact")
    idx = pick(batch)
    want = r.expect(idx)
    fast, slow = r.hist(dev, idx), r.hist(dev, idx, fast=False)
    show(f"{name} exact, {batch} boards,", r.sites, fast)
    assert np.array_equal(fast, want), np.argwhere(fast != want)[:8]
    assert np.array_equal(slow, want), np.argwhere(slow != want)[:8]
    binades = (want[:, 1:95] > 0).sum(axis=1)
    assert (want[:, 0] > 0).all() and (binades >= 2).all(), (want[:, 0], binades)
    assert (want[:, 95] == 0).all()


# ---- 2. the far bins ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifts", [(24,), (-24,), (24, 24, 24)], ids=lambda s: "k" + "_".join(map(str, s)))
@pytest.mark.parametrize("name", NAMES)
def test_a_shifted_stream_moves_the_bins(dev, name, shifts):
    r = Ref.get(name, "exact")
    idx = pick(BOARDS)
    model = r.model
    for k in shifts:
        model = model.stream_shift(k)
    want = R.shift_bins(r.expect(idx), sum(shifts))
    assert np.array_equal(want[-1], r.expect(idx)[-1]) and not np.array_equal(want[0], r.expect(idx)[0])
    if sum(shifts) == 72:  # the bottom end: everything non-zero of the shifted sites is in bin 1
        assert (want[:-1, 2:95] == 0).all() and (want[:-1, 1] > 0).all()
    for fast in (True, False):
        got = model.range_histogram(dev, r.bits[idx], r.scalars_in[idx], fast=fast)
        assert np.array_equal(got, want), (fast, np.argwhere(got != want)[:8])


# ---- 3. additivity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_counts_add_up_whatever_the_split_the_place_and_the_partner(dev, name):
    r = Ref.get(name, "random")
    idx = pick(259)
    assert 100 < CHUNK < 259
    whole = r.hist(dev, idx)
    assert np.array_equal(whole, r.hist(dev, idx[:100]) + r.hist(dev, idx[100:]))
    thirteen = r.hist(dev, idx[:BOARDS])
    assert np.array_equal(thirteen, r.hist(dev, idx[:BOARDS][::-1]))
    single = np.stack([r.hist(dev, np.array([b])) for b in range(BOARDS)])  # [board, site, 96]
    times = np.bincount(idx, minlength=BOARDS).astype(np.uint64)
    assert times.sum() == 259 and times.min() >= 19
    assert np.array_equal(whole, (single * times[:, None, None]).sum(axis=0, dtype=np.uint64))
    assert np.array_equal(thirteen, single.sum(axis=0, dtype=np.uint64))


# ---- 4. random networks against the oracle --------------------------------------------------------------------------------
def near_a_boundary(x):
    """A of the docstring for one site's trace x (all boards): elements within 1e-4 * max(1, |x|) of a binade boundary, plus
    twice the non-zero elements with |x| <= 1e-4 (a zero / non-zero flip at the ReLU moves a count out of one bin and into
    another).  In float64, from the oracle's values alone."""
    a = np.abs(x.astype(np.float64)).ravel()
    nz = a[a > 0]
    delta = F32_ATOL * np.maximum(1.0, nz)
    lo = np.ldexp(1.0, np.frexp(nz)[1] - 1)  # the binade's lower boundary: lo <= nz < 2 lo, exactly
    near = (nz - lo <= delta) | (2 * lo - nz <= delta)
    return int(near.sum()) + 2 * int((nz <= F32_ATOL).sum())


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", NAMES)
def test_random_networks_within_the_boundary_count(dev, name, batch):
    r = Ref.get(name, "random")
    idx = pick(batch)
    want = r.expect(idx)
    for fast in (True, False):
        got = r.hist(dev, idx, fast=fast)
        for site in range(len(r.sites)):
            bound = int(r.near()[site, idx].sum())
            elems = len(idx) * r.per_board_elems
            diff = int(np.abs(got[site].astype(np.int64) - want[site].astype(np.int64)).sum())
            print(f"[range hist] {name} random, {batch} boards, {'fast' if fast else 'per layer'}, {r.sites[site]}: "
                  f"sum |d| = {diff}, A = {bound} ({100.0 * bound / elems:.2f} % of {elems})")
            assert bound <= 0.01 * elems
            assert diff <= 2 * bound


# ---- 5. non-finite values -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad_value", [np.inf, -np.inf, np.nan])
def test_a_non_finite_board_fills_bin_95_and_touches_no_other(dev, bad_value):
    r = Ref.get("ataxx7x128", "random")  # two boards per workgroup: board 5 shares its workgroup with board 4
    bad = 5
    scalars_in = r.scalars_in.copy()
    scalars_in[bad, 0] = bad_value
    everyone, others = np.arange(BOARDS), np.flatnonzero(np.arange(BOARDS) != bad)
    for fast in (True, False):
        all13 = r.hist(dev, everyone, fast=fast, scalars_in=scalars_in)  # (the totals hold at every site: Ref.hist)
        alone = r.hist(dev, np.array([bad]), fast=fast, scalars_in=scalars_in)
        clean = r.hist(dev, others, fast=fast)
        assert all13[0, 95] == alone[0, 95] == r.per_board_elems
        assert (clean[:, 95] == 0).all()
        assert (all13 >= alone).all() and np.array_equal(all13 - alone, clean), fast


# ---- 6. no one-launch tower -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", (13, 69))
def test_go19_takes_the_per_layer_path(dev, batch):
    r = Ref.get("go19x64", "random")
    assert r.model.range_profile_fast_path() == "conv_igemm_f32"
    idx = pick(batch)
    assert np.array_equal(r.hist(dev, idx), r.hist(dev, idx, fast=False))


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", ["kz_model_range_histogram", "kz_model_range_histogram_fast"])
def test_refusals_carry_each_functions_name(dev, fn):
    lib = capi.load()
    bits, scalars = np.zeros((1, 512), np.uint8), np.zeros((1, 16), np.float32)
    out = np.zeros((64, capi.KZ_RANGE_BINS), np.uint64)

    def call(model, batch=1, stride=512, dest=out):
        rc = getattr(lib, fn)(model._h, dev, bits.ctypes.data, stride, scalars.ctypes.data, batch, dest.ctypes.data if dest is not None else None)
        assert rc != 0
        return lib.kz_last_error().decode()

    attention = capi.Model(blob=O.load_blob("chess_att2x64"))
    dense = capi.Model(blob=O.load_blob("sttt_dn1x64"))
    stem_only = capi.Model(blob=synth.random_model("chess", 0, 64, "attention", seed=1))
    messages = []
    for model, needle in ((attention, "ResTower"), (dense, "ResTower"), (stem_only, "without blocks")):
        messages.append(call(model))
        assert messages[-1].startswith(fn + ": ") and needle in messages[-1], messages[-1]
    res = Ref.get("ataxx7x128", "random").model
    messages += [call(res, batch=0), call(res, batch=-3), call(res, stride=3), call(res, dest=None)]
    assert messages[-4] == messages[-3] == fn + ": batch must be positive"
    assert messages[-2] == fn + ": bits_stride too small"
    assert messages[-1] == fn + ": null argument"
    assert not any("KZ_" in m for m in messages)
    assert (out == 0).all()  # a refused call writes nothing


# ---- 8. ordinary engines are untouched ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ataxx7x128", "chess256"])
def test_engines_and_the_max_profile_return_what_they_returned_before(dev, name):
    r = Ref.get(name, "random")
    want = next(s for s in SHAPES if s[0] == name)[5]
    eng = capi.Engine(r.model, dev, 64, capi.KZ_DTYPE_F32)
    assert eng.tower_path == want
    before = eng.eval_packed(r.bits, r.scalars_in)
    profile_before = r.model.range_profile_fast(dev, r.bits, r.scalars_in)
    everyone = np.arange(BOARDS)
    fast, slow = r.hist(dev, everyone), r.hist(dev, everyone, fast=False)
    assert (fast[:, 95] == 0).all() and (slow[:, 95] == 0).all()
    after = eng.eval_packed(r.bits, r.scalars_in)
    assert eng.tower_path == want
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    fresh = capi.Engine(r.model, dev, 64, capi.KZ_DTYPE_F32).eval_packed(r.bits, r.scalars_in)
    assert np.array_equal(before[0], fresh[0]) and np.array_equal(before[1], fresh[1])
    profile_after = r.model.range_profile_fast(dev, r.bits, r.scalars_in)
    assert np.array_equal(profile_before[0], profile_after[0]) and np.array_equal(profile_before[1], profile_after[1])
