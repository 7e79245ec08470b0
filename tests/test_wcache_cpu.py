"""What the weighted planned pairs of the cache rest on, without a device.

1. The +-0 identity behind cache_update_planned_kernel<.., WEIGHTED>'s skipping of dead occurrences (csrc/cache_block.hip): a
   key's chain acc = fl(acc + t_i) over ALL its occurrences, where a dead occurrence contributes z = fl(scale * +0) = +-0, equals
   the chain over the LIVE occurrences followed by ONE add of z whenever at least one dead occurrence exists, and the live chain
   alone when none does.  By bit view, float32, ~10^4 random chains: initial value +-0 / normal / tiny, live terms that include
   -0.0, exact cancellations and subnormals, dead positions anywhere.
2. The refusals that need no device: Config's default, run_wdl.train with and without the flag, the command line."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "ctr"))


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def _chain(acc, terms):
    acc = np.float32(acc)
    for t in terms:
        acc = np.float32(acc + np.float32(t))
    return acc


def _draw_chain(rng):
    tiny = np.float32(1e-45)        # the smallest subnormal
    init = rng.choice(np.array([0.0, -0.0, 1.5, -3.25e-3, tiny, -tiny, 1e-38], dtype=np.float32))
    if rng.random() < 0.3:
        init = np.float32(rng.standard_normal())
    n = int(rng.integers(1, 12))
    live = []
    for _ in range(n):
        kind = rng.integers(0, 6)
        if kind == 0:
            live.append(np.float32(-0.0))
        elif kind == 1:
            live.append(np.float32(0.0) * np.float32(rng.choice([1.0, -1.0])))       # a live term that is +-0 (g == 0)
        elif kind == 2 and live:
            live.append(np.float32(-live[-1]))                                        # an exact cancellation of the term before
        elif kind == 3:
            live.append(np.float32(rng.choice([tiny, -tiny, 3 * tiny, 1e-39, -1e-39])))
        elif kind == 4:
            live.append(np.float32(-init))                                            # cancels the initial value (if first)
        else:
            live.append(np.float32(rng.standard_normal()))
    ndead = int(rng.integers(0, 6))
    # positions of the dead occurrences among the live ones
    order = np.array([1] * len(live) + [0] * ndead)
    rng.shuffle(order)
    return init, live, order


@pytest.mark.parametrize("z", [0.0, -0.0])
def test_the_chain_over_all_terms_is_the_live_chain_and_one_add_of_z(z):
    z = np.float32(z)
    rng = np.random.default_rng(20 if np.signbit(z) else 21)
    seen = {"dead": 0, "none": 0, "minus_zero_kept": 0, "minus_zero_lost": 0}
    with np.errstate(all="ignore"):
        for _ in range(10000):
            init, live, order = _draw_chain(rng)
            it = iter(live)
            every = [next(it) if o else z for o in order]
            want = _chain(init, every)
            got = _chain(init, live)
            if (order == 0).any():
                got = np.float32(got + z)
                seen["dead"] += 1
            else:
                seen["none"] += 1
            assert _bits(got) == _bits(want), (init, live, order.tolist(), z, got, want)
            if (order == 0).any() and _bits(_chain(init, live)) == _bits(np.float32(-0.0)):
                seen["minus_zero_kept" if np.signbit(want) else "minus_zero_lost"] += 1
    assert seen["dead"] > 1000 and seen["none"] > 100, seen
    # the one case the rule is about: a live chain that ends at -0 -- one +0 term makes it +0, -0 terms leave it
    assert seen["minus_zero_lost" if not np.signbit(z) else "minus_zero_kept"] > 0, seen
    assert seen["minus_zero_kept" if not np.signbit(z) else "minus_zero_lost"] == 0, seen


def test_step_form_of_the_add_is_the_add():
    """The accumulate runs acc - fl(-1 * t) (step<kModeSgd> with lr = -1): the same bits as acc + t, signed zeros included."""
    vals = np.array([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 3.5, -2.25e-7], dtype=np.float32)
    for a in vals:
        for t in vals:
            assert _bits(np.float32(a - np.float32(np.float32(-1.0) * t))) == _bits(np.float32(a + t)), (a, t)


def test_z_is_plus_zero_for_scale_at_least_zero_and_minus_zero_below():
    for scale, neg in ((1.0, False), (0.01, False), (0.0, False), (-0.01, True), (-1.0, True)):
        z = np.float32(scale) * np.float32(0.0)
        assert z == 0 and bool(np.signbit(z)) == neg


def test_config_default_is_off():
    from herald_amd import hetu_ops
    assert hetu_ops.Config().cache_fuse_wbags is False
    assert hetu_ops.Config(cache_fuse_wbags=True).cache_fuse_wbags is True


def test_the_cache_methods_exist_on_both_classes():
    from herald_amd import cache as hcache
    for cls in (hcache.LRUCache, hcache.LFUCache, hcache.LFUOptCache, hcache.CacheSparseTable):
        for name in ("embedding_lookup_wsum_planned", "embedding_update_planned_wbags", "run_planned_pairs_wbags"):
            assert callable(getattr(cls, name)), (cls, name)


def test_run_wdl_train_refuses_fae_wdl_on_the_cache_outside_the_planned_pairs():
    import run_wdl
    kw = dict(rows=500, width=8, batch=4, steps=2, lr=0.05, device="cuda:0", model="fae_wdl")
    with pytest.raises(ValueError, match="fae_wdl.*cache-fuse-wbags"):
        run_wdl.train("cache", **kw)                                                        # without the flag
    with pytest.raises(ValueError, match="fae_wdl"):
        run_wdl.train("cache", cache_planned=True, bsp=0, **kw)                              # still without it
    with pytest.raises(ValueError, match="fae_wdl"):
        run_wdl.train("cache", cache_fuse_wbags=True, bsp=0, **kw)                           # the flag, not planned
    with pytest.raises(ValueError, match="fae_wdl"):
        run_wdl.train("cache", cache_fuse_wbags=True, cache_planned=True, bsp=-1, **kw)      # the flag, the asp chain
    for embedding in ("step", "step3", "queue"):
        with pytest.raises(ValueError, match="fae_wdl"):
            run_wdl.train(embedding, cache_fuse_wbags=True, cache_planned=True, bsp=0, **kw)
    with pytest.raises(ValueError, match="fae_deepfm"):
        run_wdl.train("cache", cache_fuse_wbags=True, cache_planned=True, bsp=0, **dict(kw, model="fae_deepfm"))


@pytest.mark.parametrize("extra", [[], ["--cache-planned", "--bsp", "-1"], ["--cache-planned"]])
def test_the_command_line_refuses_the_flag_outside_the_planned_pairs(monkeypatch, capsys, extra):
    """--cache-fuse-wbags without --cache-planned, with --bsp -1, and at the command line's default bsp (asp)."""
    import run_wdl
    monkeypatch.setattr(sys, "argv", ["run_wdl.py", "--model", "fae_wdl", "--comm", "Hybrid", "--cache", "lfu", "--bound", "0",
                                      "--cache-fuse-wbags"] + extra)
    with pytest.raises(SystemExit):
        run_wdl.main()
    # (the new check's own words: an unknown-argument error would name the flag too)
    assert "--cache-fuse-wbags needs --embedding cache, --cache-planned and --bsp 0" in capsys.readouterr().err
