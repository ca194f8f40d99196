"""The tower taps (kz_model_tower_taps) held to the bits of the float64 reference, site by site.

tests/test_gpu_exact.py holds the OUTPUTS of every launch to the reference; here every stored tensor of every one-launch tower
— the stem's output, each block's mid activation and output, the tower output behind the final BN — must equal
`exact_nets.reference`'s `report.acts[...]` bit for bit, so a wrong row, tile, partner board or residual names its layer.
The rows below reach every kernel that has a tap instance: kz_tower.hip with two boards per workgroup (and a missing partner),
with one, and with the wide stem; the split, plain-f16, bf16 and exact-f32 towers at 1, 2, 3 and 4 boards per workgroup, with
16-row tiles that boards do not fill and with a last workgroup that is part-filled.  One dense position per row beside the
all-narrow network.  The wide family puts non-zero lo halves into the split taps (`hi + lo`); the rounding family holds the
bf16 taps to a reference that rounds where the plain bf16 launch does.
"""
import contextlib
import os

import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import exact_nets as E

pytestmark = pytest.mark.gpu

F16, F32, SPLIT, BF16 = capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F32_SPLIT16, capi.KZ_DTYPE_BF16

# (id, network, dtype, max_batch, batch, switches, the tap path)
ROWS = [
    ("chess256-f16-nb2", "chess_2x256_att", F16, 64, 5, {}, "tower_resident_f16"),                    # NB = 2, a missing partner
    ("chess256-f16-nb1", "chess_2x256_att", F16, 64, 3, {"KZ_TOWER_NB": "1"}, "tower_resident_f16"),  # NB = 1
    ("chesshist1-f16", "chesshist1_1x256_att", F16, 64, 5, {}, "tower_resident_f16"),                 # the wide stem
    ("chess256-split16", "chess_2x256_att", SPLIT, 64, 9, {}, "tower_resident_split16"),
    ("chess256-f32", "chess_2x256_att", F32, 64, 9, {}, "tower_resident_f32"),
    ("chess128-f16g-1", "chess_1x128_att", F16, 64, 3, {}, "tower_resident_f16g"),
    ("chess128-f16g-2", "chess_1x128_att", F16, 256, 9, {}, "tower_resident_f16g"),                   # two boards per workgroup
    ("chess128-f16g-4", "chess_1x128_att", F16, 2048, 9, {}, "tower_resident_f16g"),                  # four; the last holds one
    ("chess192-f16g-2", "chess_1x192_att", F16, 256, 9, {}, "tower_resident_f16g"),                   # the other channel mapping
    ("chess192-split16", "chess_1x192_att", SPLIT, 64, 9, {}, "tower_resident_split16"),
    ("ataxx7x128-f16g-2", "ataxx7_1x128", F16, 64, 5, {}, "tower_resident_f16g"),                     # 49 pixels in 16-row tiles
    ("ataxx7x128-f16g-4", "ataxx7_1x128", F16, 512, 9, {}, "tower_resident_f16g"),
    ("ataxx7x128-split16", "ataxx7_1x128", SPLIT, 64, 5, {}, "tower_resident_split16"),
    ("ataxx7x128-f32", "ataxx7_1x128", F32, 64, 5, {}, "tower_resident_f32"),
    ("ataxx5x128-f16g", "ataxx5_1x128", F16, 64, 9, {}, "tower_resident_f16g"),                       # four 5x5 boards
    ("go9x128-f16g-1", "go9_1x128", F16, 64, 3, {}, "tower_resident_f16g"),
    ("go9x128-f16g-2", "go9_1x128", F16, 256, 9, {}, "tower_resident_f16g"),
    ("go9x128-f16g-3", "go9_1x128", F16, 2048, 10, {}, "tower_resident_f16g"),                        # three 9x9 boards
    ("go9x256-f16g", "go9_1x256", F16, 64, 9, {}, "tower_resident_f16g"),
    ("chess512-f16g", "chess_1x512_att", F16, 64, 9, {}, "tower_resident_f16g"),
    ("ataxx7x64-f16g", "ataxx7_1x64", F16, 64, 9, {}, "tower_resident_f16g"),
]


def dense_position(net, i):
    """One tower convolution of the network, by the row's index: the dense layer of the row's second model."""
    depth = E.NETS[net][1]
    return i % (2 * depth + 1)


# (ordered by network and position: exact_nets.build keeps the last few models)
CASES = sorted(((row, pos) for i, row in enumerate(ROWS) for pos in (None, dense_position(row[1], i))),
               key=lambda c: (list(E.NETS).index(c[0][1]), -1 if c[1] is None else c[1]))
IDS = [f"{row[0]}-{'none' if pos is None else pos}" for row, pos in CASES]

# the wide family: every network of WIDE_NETS among the rows, in split arithmetic, the stem's weights wide (lo halves in every site behind)
WIDE_ROWS = [(net, 64, 5 if net == "ataxx7_1x128" else 9) for net in E.WIDE_NETS if any(r[1] == net for r in ROWS)]


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


@contextlib.contextmanager
def switches(env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def where(out, ref):
    bad = np.argwhere(out != ref)
    pick = lambda axis: sorted(set(int(v) for v in bad[:, axis]))[:10]  # noqa: E731
    return (f"{len(bad)} of {out.size} differ, {int(np.isnan(out).sum())} never written; boards {pick(0)}, channels {pick(1)}, "
            f"rows {pick(2)}, columns {pick(3)}")


def taps_equal_reference(dev, blob, bits, scalars_in, acts, dtype, max_batch, batch, env, path, label):
    model = capi.Model(blob=blob)
    idx = np.arange(3, 3 + batch) % len(bits)  # (distinct boards, no workgroup starts the cycle)
    with switches(env):
        assert model.tower_taps_path(max_batch, dtype) == path
        taps = model.tower_taps(dev, max_batch, dtype, bits[idx], scalars_in[idx])
    names = model.range_sites()
    assert list(taps) == names and set(names) <= set(acts)
    for name in names:
        ref = acts[name][idx].astype(np.float32)
        assert np.array_equal(ref.astype(np.float64), acts[name][idx]), f"{name}: the reference is f32"
        assert np.array_equal(taps[name], ref), f"[{label}] {name}: " + where(taps[name], ref)


@pytest.mark.parametrize("row,pos", CASES, ids=IDS)
def test_taps_equal_the_reference_bits_at_every_site(dev, row, pos):
    name, net, dtype, max_batch, batch, env, path = row
    b = E.build(net, pos)
    taps_equal_reference(dev, b.blob, b.bits, b.scalars_in, b.report.acts, dtype, max_batch, batch, env, path, f"{name} dense_at={pos}")


@pytest.mark.parametrize("net,max_batch,batch", WIDE_ROWS, ids=[r[0] for r in WIDE_ROWS])
def test_split_taps_are_hi_plus_lo_on_a_wide_network(dev, net, max_batch, batch):
    wide = next(w for w in E.wide_positions(net) if w[0] == 0)
    b = E.build(net, None, wide)
    assert any(np.any(v) for v in b.report.lo_w.values()), "the wide stem weights have lo halves"
    taps_equal_reference(dev, b.blob, b.bits, b.scalars_in, b.report.acts, SPLIT, max_batch, batch, {}, "tower_resident_split16", f"{net} {E.wide_id(wide)}")


@pytest.mark.parametrize("net", sorted(E.ROUND_NETS))
def test_bf16_taps_equal_the_rounding_reference_bits(dev, net):
    """The input variant rounds at every site.  A tap instance is the plain tower, so the reference rounds where the launch
    WITHOUT heads does (bf16_sites(meta, False)): the last site is the unrounded f32 tower output whatever the engine's plan."""
    b = E.build_round(net, ("input",))
    sites, weights = E.bf16_sites(b.meta, False)
    _, _, rep = E.reference(b.tensors, b.meta, b.x, exact=False, rounding=(frozenset(sites + weights), E.bf16_rne))
    plain = E.reference(b.tensors, b.meta, b.x, exact=False, rounding=(frozenset(), None))[2].values
    assert not np.array_equal(rep.values["tower.0"], plain["tower.0"]), "the stem's output is rounded in this variant: the taps are held to a reference that rounds"
    model = capi.Model(blob=b.blob)
    assert model.tower_taps_path(64, BF16) == "tower_resident_bf16g"
    taps = model.tower_taps(dev, 64, BF16, b.bits, b.scalars_in)
    names = model.range_sites()
    assert names[-1] not in sites and set(names[:-1]) <= set(sites)
    for name in names:
        assert E.f32_exact(rep.values[name]), f"{name}: the reference is f32"
        ref = rep.values[name].astype(np.float32)
        assert np.array_equal(taps[name], ref), f"{name}: " + where(taps[name], ref)


SENTINEL = np.uint32(0x7FC0DEAD)  # a NaN no kernel computes


def test_requested_sites_are_overwritten_and_nothing_else_is_touched(dev):
    b = E.build("ataxx7_1x128", None)  # (49 pixels in 16-row tiles, two boards per workgroup, five boards: a missing partner)
    model = capi.Model(blob=b.blob)
    names = model.range_sites()
    n, batch = len(names), 5
    block = batch * 128 * 49
    for first, count in ((0, n), (1, 2), (n - 1, 1), (0, 1)):
        buf = np.full((count + 2) * block, SENTINEL, np.uint32).view(np.float32)
        taps = model.tower_taps(dev, 64, F16, b.bits[:batch], b.scalars_in[:batch], first, count, out=buf[block:block + count * block])
        bits = buf.view(np.uint32)
        assert (bits[:block] == SENTINEL).all() and (bits[(count + 1) * block:] == SENTINEL).all(), (first, count)
        assert not (bits[block:(count + 1) * block] == SENTINEL).any(), (first, count)
        assert not np.isnan(buf[block:(count + 1) * block]).any(), "a row no lane wrote reads as NaN"
        assert list(taps) == names[first:first + count]
        for name in taps:
            assert np.array_equal(taps[name], b.report.acts[name][:batch].astype(np.float32)), name


def test_every_refusal_has_its_own_text(dev):
    good = capi.Model(blob=synth.random_model("chess", 1, 128, "attention", seed=1))
    bits, scalars = synth.random_boards("chess", 4, seed=1)
    out = np.zeros(3 * 4 * 128 * 64, np.float32)
    lib = capi.load()

    def raw(model, max_batch=8, dtype=F16, bits_p=None, stride=None, scalars_p=None, batch=4, first=0, count=3, out_p=None, b=bits, s=scalars):
        rc = lib.kz_model_tower_taps(model._h if model else None, dev, max_batch, dtype, b.ctypes.data if bits_p is None else bits_p,
                                     b.shape[1] if stride is None else stride, s.ctypes.data if scalars_p is None else scalars_p, batch,
                                     first, count, out.ctypes.data if out_p is None else out_p)
        assert rc != 0
        msg = lib.kz_last_error().decode()
        assert msg.startswith("kz_model_tower_taps: "), msg
        return msg

    def other(game, depth, channels, head, **kw):
        m = capi.Model(blob=synth.random_model(game, depth, channels, head, seed=1, **kw))
        bb, ss = synth.random_boards(game, 4, seed=1)
        return dict(model=m, b=bb, s=ss)

    cases = {
        "attention tower": raw(**other("chess", 1, 64, "attention", attention=(4, 16, 16, 96))),
        "dense network": raw(**other("sttt", 1, 64, "none", dense_network=False)),
        "no blocks": raw(**other("chess", 0, 128, "attention")),
        "per layer": raw(**other("go-19", 1, 64, "conv")),
        "dtype not supported": raw(dtype=BF16, **other("go-19", 1, 64, "conv")),
        "site range": raw(good, first=2, count=2),
        "batch < 1": raw(good, batch=0),
        "batch > max_batch": raw(good, max_batch=3),
        "null argument": raw(good, out_p=0),
        "bits_stride": raw(good, stride=bits.shape[1] - 1),
    }
    assert "KZ_KEEP_ACTIVATIONS" in cases["per layer"]
    assert cases["batch < 1"] != cases["batch > max_batch"]
    assert len(set(cases.values())) == len(cases), cases
    assert raw(None) == cases["null argument"]
    # ... and the call itself works on that model
    assert list(good.tower_taps(dev, 8, F16, bits, scalars)) == good.range_sites()
