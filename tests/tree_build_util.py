"""Helpers of the flx_tree_build_device tests: seeded triangle soups, each the smallest that reaches a branch of the builder (csrc/flx_mesh.hip: split), their way
through the host builder (an OBJ text -> flx_mesh_import_obj + flx_mesh_flatten), and level_build: the level-by-level formulation csrc/flx_build.hip's kernels
implement, restated in plain numpy and float64.  A soup is float32 [n, 3, 3]: the three vertices of every triangle as its geometry row holds them."""
import functools
import gzip
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_BIAS = 100.0 * 2.0 ** -16
MIN_WIDTH = 1.0 / 256.0
LEAF_MAX = 4


# ---- soups ----------------------------------------------------------------------------------------------------------------------------------------------

def random_soup(n, seed, centre=(0.5, 0.5, 0.5), extent=0.5, size=0.05):
    """n small triangles, their first vertex uniform in a cube of half-width `extent` about `centre`"""
    rng = np.random.default_rng(seed)
    a = np.asarray(centre) + rng.uniform(-extent, extent, (n, 1, 3))
    return (a + np.concatenate([np.zeros((n, 1, 3)), rng.uniform(-size, size, (n, 2, 3))], axis=1)).astype(np.float32)


def grid_soup():
    """4 x 4 x 4 cells, a triangle across each: every bound is an integer and every centre of a bounding (-bias .. 4 + bias, then 2 .. 4 + bias, ..) one too, so
    triangles touch the centre from both sides: `<=` puts the one whose min is the centre into the first bucket"""
    cells = np.array([(i, j, k) for i in range(4) for j in range(4) for k in range(4)], np.float32)
    return np.stack([cells, cells + [1, 1, 0], cells + [0, 1, 1]], axis=1).astype(np.float32)


def flat_sheet_soup():
    """all z equal: the z axis never has room"""
    soup = random_soup(100, 3)
    soup[:, :, 2] = 0.25
    return soup


def thin_soup():
    """20 triangles within 0.004 on every axis: with the bias on both sides no half is wider than 1 / 256, so no axis has room: one leaf of 20"""
    return random_soup(20, 4, extent=0.001, size=0.001)


def duplicates_soup():
    return np.repeat(np.float32([[[0.1, 0.2, 0.3], [0.9, 0.3, 0.2], [0.4, 0.8, 0.7]]]), 9, axis=0)


def axis_tie_soup():
    """eight triangles that all straddle the x centre and form four clusters in (y, z): no straddler on y, none on z: the last axis wins, and a split on y would order
    the clusters otherwise"""
    rng = np.random.default_rng(6)
    soup = []
    for y, z in ((0, 0), (1, 0), (0, 1), (1, 1)):
        for _ in range(2):
            jitter = rng.uniform(0, 0.1, (3, 3))
            soup.append(np.array([[0.0, y, z], [1.0, y, z], [0.5, y, z]]) + jitter)
    return np.float32(soup)


def chain_soup():
    """six triangles that each span the cube: every one straddles every centre, one bucket takes them all level after level"""
    rng = np.random.default_rng(8)
    soup = [np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.9], [0.2, 1.0, 0.5]]) + rng.uniform(0, 0.05, (3, 3)) for _ in range(6)]
    return np.float32(soup)


def many_chains_soup():
    """4 x 4 x 4 well-separated clusters of six cube-spanning triangles: the grid splits into its clusters within six levels, and each cluster then chains single
    children down to the depth limit: more boxes than triangles + 64, which is where the device's node arrays start: they must grow in the middle of the build"""
    rng = np.random.default_rng(10)
    soup = [np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.9], [0.2, 1.0, 0.5]]) + rng.uniform(0, 0.05, (3, 3)) + 4.0 * np.array([i, j, k])
            for i in range(4) for j in range(4) for k in range(4) for _ in range(6)]
    return np.float32(soup)


def depth_limit_soup():
    """five unit triangles at the origin and one triangle at x = 2^k for k = 3 .. 26: every level peels the farthest one off until the depth limit ends it"""
    rng = np.random.default_rng(9)
    soup = [np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 1.0]]) + rng.uniform(0, 0.1, (3, 3)) for _ in range(5)]
    soup += [np.array([[2.0 ** k, 0.0, 0.0], [2.0 ** k, 1.0, 0.0], [2.0 ** k, 0.0, 1.0]]) for k in range(3, 27)]
    return np.float32(soup)


SOUPS = {
    "n1": lambda: random_soup(1, 11), "n4": lambda: random_soup(4, 12), "n5": lambda: random_soup(5, 13),
    "n255": lambda: random_soup(255, 14), "n256": lambda: random_soup(256, 15), "n257": lambda: random_soup(257, 16),
    "n65537": lambda: random_soup(65537, 17, size=0.01),
    "centre_ties": grid_soup, "flat_sheet": flat_sheet_soup, "thin": thin_soup, "duplicates": duplicates_soup, "axis_tie": axis_tie_soup,
    "chain": chain_soup, "many_chains": many_chains_soup, "depth_limit": depth_limit_soup,
}
TRANSFORM_OF = {"n257": 5}                                          # one soup stands in another object space than 0


@functools.lru_cache(maxsize=None)
def soup(name):
    s = SOUPS[name]()
    s.setflags(write=False)
    return s


# ---- the host builder -----------------------------------------------------------------------------------------------------------------------------------

def obj_text(soup):
    """an OBJ of the soup: %.9g round-trips a float32 through the importer's one rounding; a face lists its corners backwards, as the importer reads them"""
    lines = ["v %.9g %.9g %.9g" % tuple(v) for v in soup.reshape(-1, 3).astype(np.float64)]
    lines += ["f %d %d %d" % (3 * k + 3, 3 * k + 2, 3 * k + 1) for k in range(soup.shape[0])]
    return "\n".join(lines) + "\n"


def block_of_text(text, transform=0):
    from flexlight_hip import capi
    mesh = capi.Mesh(text)
    if transform:
        mesh.set_transform(transform)
    g, a, ids, _ = mesh.flatten()
    mesh.close()
    return g, a, ids


def host_block(soup, transform=0):
    """(geometry [entries, 12], attributes [entries, 28], ids [n]) of flx_mesh_import_obj + flx_mesh_flatten"""
    return block_of_text(obj_text(soup), transform)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def entry_of_face(block, soup):
    """the block's entry that holds face k's triangle, by the bits of its nine vertex words (equal faces: in the block's order)"""
    g, _, ids = block
    where = {}
    for e in ids[::-1]:
        where.setdefault(bits(g[e, :9]).tobytes(), []).append(int(e))
    out = np.array([where[bits(face).tobytes()].pop() for face in soup.reshape(-1, 9)], np.int64)
    assert np.array_equal(np.sort(out), np.sort(ids))
    return out


def face_order_rows(block, soup):
    """the block's triangle rows (geometry [n, 12], attributes [n, 28]) in face order: what the device builder is given"""
    at = entry_of_face(block, soup)
    return block[0][at].copy(), block[1][at].copy()


@functools.lru_cache(maxsize=None)
def case(name):
    """(soup, the host's block, its triangle rows in face order), made once"""
    s = soup(name)
    block = host_block(s, TRANSFORM_OF.get(name, 0))
    rows = face_order_rows(block, s)
    for a in block + rows:
        a.setflags(write=False)
    return s, block, rows


def soup_of_obj(text):
    """the soup of an OBJ whose faces have three corners, in face order, as the importer reads it (corners backwards, vertex indices from 1 or from the end)"""
    vertices, faces = [], []
    for line in text.splitlines():
        w = line.split()
        if w and w[0] == "v":
            vertices.append([float(x) for x in w[1:4]])
        elif w and w[0] == "f":
            assert len(w) == 4, line
            idx = [int(c.split("/")[0]) for c in w[1:]]
            faces.append([vertices[i - 1 if i > 0 else len(vertices) + i] for i in idx[::-1]])
    return np.asarray(faces, np.float64).astype(np.float32)


def asset_text_in_triangles(name):
    """tests/golden/assets/objects/<name>.obj.gz with every four-cornered face rewritten as two three-cornered ones"""
    with gzip.open(os.path.join(ROOT, "tests", "golden", "assets", "objects", name + ".obj.gz"), "rt") as f:
        lines = f.read().splitlines()
    out = []
    for line in lines:
        w = line.split()
        if w and w[0] == "f" and len(w) == 5:
            out += ["f %s %s %s" % (w[1], w[2], w[3]), "f %s %s %s" % (w[1], w[3], w[4])]
        else:
            out.append(line)
    return "\n".join(out) + "\n"


# ---- the level-by-level formulation ---------------------------------------------------------------------------------------------------------------------

def exclusive(flags):
    """the exclusive scan, one item longer than its input: its last item is the total"""
    return np.concatenate([[0], np.cumsum(flags, dtype=np.int64)])


def level_build(soup):
    """-> (kind [entries], skip [entries] (boxes), face [entries] (triangles; -1: a box), ids [n]).  Arrays per position and per node, one round per level, as the
    kernels go: a node owns a range of the permutation; the later triangles' min / max per node; centre and room; straddlers per axis; the axis; buckets; ranks
    from scans of the flags minus their value at the node's start; children in the order of their parents; open; and the index formula at the end."""
    v = np.asarray(soup, np.float32).astype(np.float64)
    n = v.shape[0]
    lo, hi = v.min(axis=1), v.max(axis=1)
    max_depth = np.log2(float(n)) + 8.0
    perm = np.arange(n)
    owner = np.zeros(n, np.int64) if n > LEAF_MAX else np.full(n, -1, np.int64)
    first, count, r = np.array([0]), np.array([n]), np.array([0])
    open_ = np.zeros(n + 1, np.int64)
    open_[0] = 1
    base, m, depth = 0, 1, 0
    while True:
        f, c = first[base:base + m], count[base:base + m]
        live = (c > LEAF_MAX) & (not depth > max_depth)
        centre = np.zeros((m, 3))
        room = np.zeros((m, 3), bool)
        if live.any():
            # the node's bounding: its first triangle's own, joined with the later ones' widened by the bias
            ends = np.stack([f[live] + 1, f[live] + c[live]], axis=1).reshape(-1)
            later_lo = np.minimum.reduceat(np.vstack([lo[perm], np.full((1, 3), np.inf)]), ends, axis=0)[::2]
            later_hi = np.maximum.reduceat(np.vstack([hi[perm], np.full((1, 3), -np.inf)]), ends, axis=0)[::2]
            blo = np.minimum(lo[perm[f[live]]], later_lo - NODE_BIAS)
            bhi = np.maximum(hi[perm[f[live]]], later_hi + NODE_BIAS)
            centre[live] = (blo + bhi) / 2.0
            room[live] = np.minimum(bhi - centre[live], centre[live] - blo) > MIN_WIDTH
        at = np.flatnonzero(owner >= 0)
        q = owner[at] - base                                        # the position's node, counted within the level
        tlo, thi = lo[perm[at]], hi[perm[at]]
        axis = np.full(m, -1)
        fewest = np.zeros(m, np.int64)
        for a in range(3):
            straddles = ~(centre[q, a] <= tlo[:, a]) & ~(centre[q, a] >= thi[:, a])
            counted = np.bincount(q[straddles], minlength=m)
            take = room[:, a] & ((axis < 0) | (fewest >= counted))
            axis[take], fewest[take] = a, counted[take]
        bucket = np.full(n, 3)
        splits = axis[q] >= 0
        p, qa = at[splits], q[splits]
        ca = centre[qa, axis[qa]]
        bucket[p] = np.where(ca <= lo[perm[p], axis[qa]], 0, np.where(ca >= hi[perm[p], axis[qa]], 1, 2))
        x0, x1 = exclusive(bucket == 0), exclusive(bucket == 1)
        n0 = np.where(axis >= 0, x0[f + c] - x0[f], 0)
        n1 = np.where(axis >= 0, x1[f + c] - x1[f], 0)
        n2 = np.where(axis >= 0, c - n0 - n1, 0)
        kids = (n0 > 0).astype(np.int64) + (n1 > 0) + (n2 > 0)
        y = exclusive(kids)
        children = int(y[m])
        if children == 0:
            break
        total = base + m
        first, count, r = (np.concatenate([z, np.zeros(children, np.int64)]) for z in (first, count, r))
        start, slot = f.copy(), total + y[:m]
        for size in (n0, n1, n2):
            has = size > 0
            first[slot[has]], count[slot[has]] = start[has], size[has]
            r[slot[has]] = np.where(start[has] == f[has], r[base:base + m][has] + 1, 0)
            open_[start[has]] += 1
            start, slot = start + size, slot + has
        # the stable partition
        b = bucket[p]
        r0, r1 = x0[p] - x0[f[qa]], x1[p] - x1[f[qa]]
        r2 = (p - f[qa]) - r0 - r1
        to = f[qa] + np.where(b == 0, r0, np.where(b == 1, n0[qa] + r1, n0[qa] + n1[qa] + r2))
        size = np.where(b == 0, n0[qa], np.where(b == 1, n1[qa], n2[qa]))
        child = total + y[qa] + np.where(b == 0, 0, (n0[qa] > 0).astype(np.int64) + ((b == 2) & (n1[qa] > 0)))
        perm_next, owner_next = perm.copy(), np.full(n, -1, np.int64)
        perm_next[to] = perm[p]
        owner_next[to] = np.where(size > LEAF_MAX, child, -1)
        perm, owner = perm_next, owner_next
        base, m, depth = total, children, depth + 1
    nodes = first.size
    before = exclusive(open_[:n])                                   # (n + 1 items)
    triangle_entry = np.arange(n) + before[:n] + open_[:n]
    node_entry = first + before[first] + r
    beneath = count + (before[first + count] - before[first]) - r - 1
    kind = np.zeros(n + nodes, np.int64)
    skip = np.zeros(n + nodes, np.int64)
    face = np.full(n + nodes, -1, np.int64)
    kind[triangle_entry], face[triangle_entry] = 2, perm
    assert (kind[node_entry] == 0).all()
    kind[node_entry], skip[node_entry] = 1, beneath
    return kind, skip, face, triangle_entry.astype(np.int32)
