"""The synthetic scene generator feeds well-formed arrays and the oracle is deterministic on them (CPU only)."""
import numpy as np
import pytest

import synth_scene


def test_generator_is_well_formed_and_oracle_is_thread_independent(oracle):
    sc = synth_scene.make(seed=11, n_objects=4, tris_per_object=20, n_transforms=4, n_lights=2, width=48, height=32)
    g = sc.arrays["geometry"].reshape(-1, 12)
    n = g.shape[0]
    assert n % 256 == 0
    for i in np.flatnonzero(g[:, 10] == 1):
        assert i + g[i, 6] < n and g[i, 6] >= 1
        inside = g[i + 1:i + 1 + int(g[i, 6])]
        tris = inside[inside[:, 10] == 2][:, :9].reshape(-1, 3)
        assert (tris >= g[i, 0:3] - 1e-6).all() and (tris <= g[i, 3:6] + 1e-6).all()
    assert set(np.unique(g[:, 10])) <= {0.0, 1.0, 2.0}
    p = sc.frame_params(use_filter=0)
    a, ca, _ = oracle.render(sc, p, threads=1)
    b, cb, _ = oracle.render(sc, p, threads=4)
    assert np.array_equal(a, b, equal_nan=True) and ca == cb
    assert ca["primary_hits"] > 0 and ca["shadow_walks"] > 0 and ca["atlas_texels"] > 0


def test_no_terminator_scene_has_none(oracle):
    sc = synth_scene.make(seed=4, n_objects=3, tris_per_object=50, n_transforms=3, n_lights=1, exact_multiple=True, width=32, height=24)
    g = sc.arrays["geometry"].reshape(-1, 12)
    assert (g[:, 10] != 0).all()
    img, cnt, _ = oracle.render(sc, sc.frame_params(use_filter=0))
    assert cnt["primary_hits"] > 0 and np.isfinite(img[..., 3]).all()


def _well_formed(g):
    n = g.shape[0]
    assert n % 256 == 0
    assert set(np.unique(g[:, 10])) <= {0.0, 1.0, 2.0}
    live = int((g[:, 10] != 0).sum())
    assert (g[:live, 10] != 0).all() and (g[live:, 10] == 0).all()            # the entries, then terminators only
    assert g[0, 10] == 1 and g[0, 6] == live - 1                               # the root box spans all of them
    for i in np.flatnonzero(g[:, 10] == 1):
        assert g[i, 6] >= 1 and i + g[i, 6] < max(n, live + 1)
        inside = g[i + 1:i + 1 + int(g[i, 6])]
        same = inside[(inside[:, 10] == 2) & (inside[:, 9] == g[i, 9])][:, :9].reshape(-1, 3)
        assert (same >= g[i, 0:3]).all() and (same <= g[i, 3:6]).all()        # (bounds in the box's own object space)
    return live


def _threaded_sizes(g):
    """walk_hot, walk_entries and fwd_entries as the library's scene upload derives them (build_threaded, build_lockstep): every non-terminator entry plus
    one shared terminator, the shallowest 4096 of them hot"""
    live = int((g[:, 10] != 0).sum())
    return min(live, 4096) + 1, live + 1, live + 1


@pytest.mark.parametrize("entries,n_transforms", [(127, 1), (128, 1), (600, 3), (4095, 1), (4096, 1), (4097, 6), (5000, 2)])
def test_sized_scene_has_exactly_its_entries(entries, n_transforms):
    sc = synth_scene.make_sized(entries, n_transforms, seed=entries)
    g = sc.arrays["geometry"].reshape(-1, 12)
    assert _well_formed(g) == entries
    assert _threaded_sizes(g) == (min(entries, 4096) + 1, entries + 1, entries + 1)
    assert sc.meta["textureLength"] == entries and sc.meta["transforms"] == n_transforms
    assert set(np.unique(g[g[:, 10] != 0, 9]).astype(int)) == set(range(n_transforms))   # every object space is used
    assert np.isfinite(g).all()
    r = sc.arrays["rotation"].reshape(-1, 24)
    for t in range(n_transforms):                                                # the inverse rotation is the inverse
        m = np.stack([r[t, 4 * k:4 * k + 3] for k in range(3)])
        mi = np.stack([r[t, 12 + 4 * k:12 + 4 * k + 3] for k in range(3)])
        assert np.allclose(m @ mi, np.eye(3), atol=1e-5)


def test_sized_scene_refuses_too_few_entries():
    with pytest.raises(ValueError):
        synth_scene.make_sized(6, 2)


@pytest.mark.parametrize("entries,n_transforms", [(128, 1), (700, 4), (4097, 2)])
def test_sized_scene_oracle_is_thread_independent_and_walks_deep(oracle, entries, n_transforms):
    sc = synth_scene.make_sized(entries, n_transforms, seed=3)
    p = sc.frame_params(use_filter=0)
    assert (p.width, p.height, p.samples, p.max_reflections) == (64, 48, 2, 3)
    a, ca, _ = oracle.render(sc, p, threads=1)
    b, cb, _ = oracle.render(sc, p, threads=4)
    assert np.array_equal(a, b, equal_nan=True) and ca == cb
    paths = p.width * p.height * p.samples
    assert ca["primary_hits"] > 0.25 * paths and ca["shadow_walks"] > 0
    assert ca["closest_visits"] > 10 * paths                                      # rays go deep into the tree, not just past its root
