"""The rounding family of tests/exact_nets.py, without a GPU: networks on which the bf16 launch does round, with a float64
reference that rounds where kz_tower_pairs.hpp rounds (`bf16_sites`), to nearest even (`bf16_rne`).

Per case: the family's conditions hold with no seed redraw — every sum within 2^22 steps, every value in front of a rounding and
every stored tensor finite and exact in f32, the outputs exact in f32 — so what the launch returns is a matter of bits in any
summation order.  Per network: every rounding site holds, over the network's cases together, COVER_TIES ties that go down,
as many that go up and COVER_OTHER values that are no tie; and every mutant reference — another direction, truncated weights,
one site less, one rounding more — returns other outputs than the rounding reference in every case it applies to.  A mutant
applies to a case when it changes some tensor the launch keeps (a stored activation or a layer's packed weights): then a
launch that did the same would be a different launch, and the outputs must say so.

What the parity bound of tests/test_gpu_bf16.py cannot see: test_truncation_fits_under_the_parity_bound.
"""
import numpy as np
import pytest

from kzero_amd import synth
from kzero_amd.model_file import read_model
from tests import exact_nets as E

COVER_TIES, COVER_OTHER = 500, 25  # per activation site and network: ties down, ties up; values that are no tie
# a layer's weights, in the variant that makes them long: every class as often as an activation site must hold values that are
# no tie.  The host's conversion is one elementwise function (the exact networks hold the layouts): what it needs is each
# class, not a count per fragment, and the Ataxx stem (3 planes x 9 taps x 128 rows) has no 500 of anything.
COVER_WEIGHTS = 25
MUTANT_MIN = 32    # output entries a mutant moves per network, all cases together

CASES = [(net, v) for net in E.ROUND_NETS for v in E.round_variants(net)]
IDS = [f"{net}-{E.round_id(v)}" for net, v in CASES]

_RESULT = {}


def case_result(net, variant):
    """(report.ties, {mutant: output entries that differ}, {mutant: it applies}) of one case; computed once."""
    if (net, variant) not in _RESULT:
        b = E.build_round(net, variant)
        moved, applies = {}, {}
        for name, rounding in E.round_mutants(b).items():
            s, p, applies[name] = E.run_mutant(b, rounding)
            moved[name] = int(np.count_nonzero(s != b.ref_scalars) + np.count_nonzero(p != b.ref_policy))
        _RESULT[net, variant] = (dict(b.report.ties), moved, applies)
    return _RESULT[net, variant]


def test_bf16_rne_from_the_definition():
    one = 2.0 ** -7  # the last of bf16's 8 significant bits at 1.0
    v = np.array([1.0, 1 + one / 2, 1 + 3 * one / 2, 1 + one / 2 + 2.0 ** -12, 1 + one - 2.0 ** -12, 1 + one, 0.0, -(1 + one / 2), -(1 + 3 * one / 2),
                  255.0, 256.5, 257.0, 259.0, 3.0 * 2.0 ** 100, (1 + 2.0 ** -8) * 2.0 ** -100, 1 + 2.0 ** -23, 2 - 2.0 ** -23, 2 - one / 2])
    rne = [1.0, 1.0, 1 + 2 * one, 1 + one, 1 + one, 1 + one, 0.0, -1.0, -(1 + 2 * one), 255.0, 256.0, 256.0, 260.0, 3.0 * 2.0 ** 100, 2.0 ** -100, 1.0, 2.0, 2.0]
    trunc = [1.0, 1.0, 1 + one, 1.0, 1.0, 1 + one, 0.0, -1.0, -(1 + one), 255.0, 256.0, 256.0, 258.0, 3.0 * 2.0 ** 100, 2.0 ** -100, 1.0, 2 - one, 2 - one]
    away = [1.0, 1 + one, 1 + 2 * one, 1 + one, 1 + one, 1 + one, 0.0, -(1 + one), -(1 + 2 * one), 255.0, 256.0, 258.0, 260.0, 3.0 * 2.0 ** 100, (1 + one) * 2.0 ** -100, 1.0, 2.0, 2.0]
    assert E.bf16_rne(v).tolist() == rne and E.bf16_trunc(v).tolist() == trunc and E.bf16_half_away(v).tolist() == away
    # a bf16 value is the upper half of its f32: every result has sixteen zero bits below
    for fn in (E.bf16_rne, E.bf16_trunc, E.bf16_half_away):
        assert not (fn(v).astype(np.float32).view(np.uint32) & 0xffff).any()
    # and the three differ where they should: on every 16-bit tail of one binade
    tails = (np.arange(1 << 16, dtype=np.uint32) | np.uint32(0x3f9d0000)).view(np.float32).astype(np.float64)
    lo, hi = np.float32(1.2265625), np.float32(1.234375)  # 0x3f9d0000 (odd last bit) and its upper neighbour
    assert set(E.bf16_rne(tails).tolist()) == {float(lo), float(hi)} and (E.bf16_trunc(tails) == lo).all()
    assert int((E.bf16_rne(tails) == lo).sum()) == 1 << 15 and int((E.bf16_half_away(tails) == lo).sum()) == 1 << 15  # the tie goes up from an odd bit
    with pytest.raises(AssertionError):
        E.bf16_rne(np.array([1.0 + 2.0 ** -30]))  # not an f32 value: the launch never rounds such a thing
    rep = E._Report()
    rep.count("x", v)
    assert rep.ties["x"] == (4, 4, 5) and rep.f32["x.before"]


def test_the_sites_are_the_kernels():
    """bf16_sites against the two shapes of the launch (kz_tower_pairs.hpp: `epilogue` into X / Y, the last layer's branch on
    HEADS, the staging's split4<E>; kz_tower_pairs_pack.hip: element_bits on the stem, the blocks and the heads' hidden pass)."""
    sites, weights = E.bf16_sites({"tower_depth": 2}, True)
    assert sites == ["input", "tower.0", "tower.1.mid", "tower.2.mid", "tower.1", "tower.3", "policy_head.hidden"]
    assert weights == ["common.tower.0", "common.tower.1.seq.0", "common.tower.1.seq.3", "common.tower.2.seq.0", "common.tower.2.seq.3", "policy_head.seq.0"]
    sites, weights = E.bf16_sites({"tower_depth": 1}, False)
    assert sites == ["input", "tower.0", "tower.1.mid"] and weights == ["common.tower.0", "common.tower.1.seq.0", "common.tower.1.seq.3"]


@pytest.mark.parametrize("net,variant", CASES, ids=IDS)
def test_conditions_and_mutants(net, variant):
    b = E.build_round(net, variant)
    rep = b.report
    print(f"[round] {net} {variant}: max sum |a b| / step = {max(rep.sums.values()):.0f}" + (f", query channels: one in {b.thin}" if b.thin else ""))
    assert b.seed == E.SEED, "the committed list needs no redraw"
    assert b.thin in (None, E.ROUND_THIN.get(b.meta.get("policy_query_channels"))), "nor more thinning"
    assert set(rep.ties) == set(b.sites) | set(b.weights) and set(b.sites) <= set(rep.f32)
    reports = [("rounded", rep)] + ([("unrounded", b.plain_report)] if variant[0] == "input" else [])
    for label, r in reports:
        for name, v in r.sums.items():
            assert v <= E.SUM_MAX, f"{label} {name}: sum |a b| / step = {v}"
        for name, ok in r.f32.items():
            assert ok, f"{label} {name}: not finite, or not exact in f32"
    # (reference() itself asserts that the outputs are exact in f32)
    for s64, p64, s32, p32 in [b.ref64 + (b.ref_scalars, b.ref_policy)]:
        assert np.array_equal(s32.astype(np.float64), s64) and np.array_equal(p32.astype(np.float64), p64)
        assert np.isfinite(s32).all() and np.isfinite(p32).all()
    for p in b.layers:
        assert b.tensors[p + ".bias"].any(), f"{p}: an all-zero bias hides a bias indexing error"
    # a second evaluation of the finished network (no revive pass) returns the same bits
    s, p, _ = E.reference(b.tensors, b.meta, b.x, rounding=b.rounding)
    assert np.array_equal(s, b.ref64[0]) and np.array_equal(p, b.ref64[1])
    if variant[0] == "input":  # it is the rounding that separates the two references
        assert int((b.plain_scalars != b.ref_scalars).sum() + (b.plain_policy != b.ref_policy).sum()) >= MUTANT_MIN
    ties, moved, applies = case_result(net, variant)
    for name, n in moved.items():
        print(f"[round]   {name}: {'applies' if applies[name] else 'the same launch'}, {n} output entries differ")
        if applies[name]:
            assert n >= 1, f"{name}: the case is blind to it"
        else:
            assert n == 0
    # the variant rounds where it says
    if variant[0] == "input":
        assert all(min(ties[s]) >= 1 for s in ("input",)), ties["input"]
    elif variant[0] == "weights":
        layer = b.layers[variant[1]]
        assert min(ties[layer]) >= COVER_WEIGHTS, (layer, ties[layer])
        assert not any(sum(ties[w]) for w in b.weights if w != layer)
        assert applies["truncated-weights"]
    else:
        assert not any(sum(ties[w]) for w in b.weights), "a dense layer times an odd gain <= 7 is a bf16 value"


@pytest.mark.parametrize("net", list(E.ROUND_NETS))
def test_coverage_and_mutants_per_network(net):
    variants = E.round_variants(net)
    results = [case_result(net, v) for v in variants]
    b = E.build_round(net, variants[0])
    n_scalar = b.meta["input_scalar_channels"]
    total = {k: np.sum([r[0][k] for r in results], axis=0) for k in b.sites}
    for site, (down, up, other) in total.items():
        print(f"[round] {net} {site}: {down} ties down, {up} ties up, {other} no tie")
        if site == "input":
            assert min(down, up, other) >= 1, site
        elif site == "tower.0" and n_scalar < 2:
            continue  # (one scalar plane: the stem's output sees that plane's factor alone)
        else:
            assert down >= COVER_TIES and up >= COVER_TIES and other >= COVER_OTHER, (site, down, up, other)
    names = set().union(*[r[1] for r in results])
    expected = {"truncate", "half-away", "branch-rounded"} | {"without-" + s for s in b.sites}
    expected |= {"truncated-weights"} if b.heads_inside else {"last-block-rounded"}
    assert expected <= names, expected - names
    for name in sorted(names):
        n = sum(r[1][name] for r in results if name in r[1])
        cases = sum(1 for r in results if r[2].get(name))
        print(f"[round] {net} mutant {name}: {n} output entries in {cases} cases")
        assert cases >= 1 and n >= MUTANT_MIN, name


def test_truncation_fits_under_the_parity_bound():
    """The gap this file closes.  On a random-weight Ataxx 2x128 — one of the plain networks of tests/test_gpu_bf16.py —
    a reference that truncates at every site stays inside the bound that holds the bf16 engine to the oracle (2.4e-2 /
    5.9e-3 of the output scale), and so does one that rounds the branch before the residual add; on the rounding family
    either changes the outputs."""
    BF16_REL, BF16_RMS = 2.4e-2, 5.9e-3  # tests/test_gpu_bf16.py (a GPU module: restated)
    meta, t = read_model(synth.random_model("ataxx-7", 2, 128, "ataxx_conv", seed=5))
    bits, scalars = synth.random_boards("ataxx-7", 13, seed=3)
    x = E.encode(meta, bits, scalars).astype(np.float32).astype(np.float64)
    s0, p0, _ = E.reference(t, meta, x, exact=False)
    sites, weights = E.bf16_sites(meta, True)
    both = frozenset(sites + weights)

    def to_f32(fn):  # (random weights: what a site sees is a float64; the launch's f32 value of it first)
        return lambda v: fn(np.asarray(v, np.float64).astype(np.float32).astype(np.float64))
    worst = {}
    for name, rounding in (("rne", (both, to_f32(E.bf16_rne))), ("truncate", (both, to_f32(E.bf16_trunc))),
                           ("branch-rounded", (both | {"tower.1.branch", "tower.2.branch"}, to_f32(E.bf16_rne)))):
        s, p, _ = E.reference(t, meta, x, exact=False, rounding=rounding)
        rel = rms = 0.0
        for a, ref in ((s, s0), (p, p0)):
            scale = np.maximum(1.0, np.abs(ref).max(axis=-1, keepdims=True))
            rel = max(rel, float((np.abs(a - ref) / scale).max()))
            rms = max(rms, float(np.sqrt(np.mean(((a - ref) / scale) ** 2))))
        worst[name] = (rel, rms)
        print(f"[gap] {name}: max |delta| / scale = {rel:.3e}, rms = {rms:.3e} (bound {BF16_REL} / {BF16_RMS})")
        assert rel <= BF16_REL and rms <= BF16_RMS, name
    assert worst["truncate"][1] > worst["rne"][1]  # it is worse, and it passes
