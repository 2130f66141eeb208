"""Scenario table of the sharded path: small clouds, each built to reach ONE branch of bs_segment_sharded's orchestration
(csrc/bs_sharded.hip) that synth.boxes() at halo 250 never takes.  The expected result of every scenario is the
one-process CPU oracle (knn_normals, then region_grow).  Whether a scenario reaches its branch depends on facts about
its cloud -- components of the kNN graph, the largest k-th distance, the extent -- which facts() computes from the
oracle's k-lists and scipy's connected components; tests/test_shard_scenarios_cpu.py asserts them without a GPU, and
tests/test_gpu_sharded_scenarios.py compares bs_shard_info with the same computed numbers.

The clouds come from synth.boxes() with small edges, the sheet helper of tests/test_gpu_knn_stream.py, lattices and
tests/golden/*.npz; 40 to 15 000 points, so that a scenario takes a second or two including the oracle."""
import os
import sys
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
GOLD = os.path.join(TESTS, "golden")
RADIUS = 100.0  # bs_params_default: the hybrid search radius


def _sheet(nx, ny, spacing, z=0):
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    from test_gpu_knn_stream import _sheet as sheet  # (imported late: the module belongs to pytest's collection)
    return sheet(nx, ny, spacing, z)


def _lattice(n, spacing):
    g = np.arange(n)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) * spacing


def _shuffled(xyz, seed):
    xyz = np.asarray(xyz)
    return np.ascontiguousarray(xyz[np.random.default_rng(seed).permutation(len(xyz))], dtype=np.int32)


# ---- clouds ----------------------------------------------------------------------------------------------------
def boxes3():
    from buildingsegment_amd import synth
    return synth.boxes(n_boxes=3, edge_lo=20, edge_hi=28)


def boxes6():
    from buildingsegment_amd import synth
    return synth.boxes(n_boxes=6, edge_lo=20, edge_hi=24)


def disc_sheet():
    """A 50 mm sheet cut to a disc, shuffled.  (A rectangle's corner points have their 16th neighbour at exactly 200 mm
    = 2 * h0: strict against non-strict comparison would decide the retry count.  On the disc the largest 16th distance
    is 158 mm, the interior's 112 mm.)"""
    s = _sheet(75, 75, 50)
    c = 37 * 50
    return _shuffled(s[(s[:, 0] - c) ** 2 + (s[:, 1] - c) ** 2 <= (36 * 50) ** 2], 41)


def disc_and_lattice400():
    """The disc and 200 points on a 400 mm lattice beside it: a lattice corner's 16th neighbour lies at 894 mm."""
    iso = _lattice(6, 400)[:200] + np.array([4400, 0, 400])
    return _shuffled(np.concatenate([disc_sheet(), iso]), 42)


def coarse_lattice():
    """7^3 points 3 m apart: a corner's 16th neighbour lies at 3 000 * sqrt(5) = 6 708 mm, beyond 64 * 100 mm."""
    return np.ascontiguousarray(_lattice(7, 3000), dtype=np.int32)


def far_boxes():
    """Two small boxes 3 000 000 mm apart in x, the first one moved 1 500 000 mm up in y: extent 3 000 000 >= 2^21.
    With the keys' shift of 1 the second box sorts last (bit 20 of x >> 1); keys cut to 21 bits without the shift would
    see it at x = 902 848 and the first box's y bit 20 would sort THAT one last -- the slabs, and with them the ranks
    that grow each box, would swap."""
    from buildingsegment_amd import synth
    xyz = synth.boxes(n_boxes=2, edge_lo=20, edge_hi=24, pitch=3_000_000).astype(np.int64)
    xyz[xyz[:, 0] < 1_000_000, 1] += 1_500_000
    return np.ascontiguousarray(xyz, dtype=np.int32)


def far_boxes_at_domain_edge():
    xyz = far_boxes().astype(np.int64)
    xyz += (1 << 23) - 2 - xyz.max()
    return np.ascontiguousarray(xyz, dtype=np.int32)


def far_boxes_negative():
    return np.ascontiguousarray(-far_boxes_at_domain_edge())


def lattice24():
    """24^3 points 40 mm apart in a fixed shuffle: equidistant candidates at the k-th place in most rows, and the
    shuffle makes the order of the global indices differ from any slab's order."""
    return _shuffled(_lattice(24, 40), 43)


def tiny40():
    """40 points in three patches of a 50 mm sheet (13 + 12 + 15) 1.45 m apart.  At world 3 the Morton slabs are exactly
    the patches (asserted from the restated partition), every one smaller than k = 16, and the patches are more than two
    halo voxels (500 mm) apart: on EVERY rank slab + halo < k until the voxels bridge the gaps -- no rank runs a kNN that
    could ask for the wider halo on its own.  (Inside a few hundred mm the first exchange would already bring all 40
    points: its voxels are never smaller than 500 mm.)"""
    p = _sheet(8, 2, 50)
    return _shuffled(np.concatenate([p[:13], p[:12] + [1450, 0, 0], p[:15] + [2900, 0, 0]]), 44)


def _golden(name):
    return np.ascontiguousarray(np.load(os.path.join(GOLD, name + ".npz"))["xyz"], dtype=np.int32)


def walls_6k():
    return _golden("walls_6k")


def plane_cube_12k():
    return _golden("plane_cube_12k")


# ---- share rules: which rank passes which points ----------------------------------------------------------------
def shares(rule, n, world):
    """-> list of `world` int32 arrays of global indices, in the order the rank passes its points"""
    idx = np.arange(n, dtype=np.int32)
    if rule == "contiguous":
        b = [(n * r) // world for r in range(world + 1)]
        out = [idx[b[r]:b[r + 1]] for r in range(world)]
    elif rule == "interleaved":
        out = [idx[r::world] for r in range(world)]
    elif rule == "random":
        a = np.random.default_rng(1000 + n + world).integers(0, world, n)
        out = [idx[a == r][::-1] for r in range(world)]  # (descending: not even sorted inside a share)
    elif rule == "rank1_nothing":
        rest = [r for r in range(world) if r != 1]
        out = [idx[:0]] * world
        for j, r in enumerate(rest):
            out[r] = idx[j::len(rest)]
    elif rule == "rank0_everything":
        out = [idx] + [idx[:0]] * (world - 1)
    else:
        raise ValueError(rule)
    return [np.ascontiguousarray(s) for s in out]


@dataclass(frozen=True)
class Scenario:
    name: str
    cloud: object          # callable -> int32 [n, 3]
    world: int
    rule: str
    halo: float            # the `halo` argument (0: the default, 2 * radius)
    k: int = 16
    rg_mode: int = 0
    components: int = 1    # of the undirected kNN graph (asserted from scipy)
    retries: object = 0    # halo doublings; None: more than six, BS_ERR_UNCERTIFIED
    shift: int = 0         # of the Morton keys
    branch: str = ""


SCENARIOS = [
    Scenario("boxes3_contiguous_w2", boxes3, 2, "contiguous", 250.0, components=3, branch="baseline at test size"),
    Scenario("boxes3_k15_w2", boxes3, 2, "interleaved", 250.0, k=15, components=3, branch="k = 15"),
    Scenario("boxes3_k32_w3", boxes3, 3, "random", 250.0, k=32, components=3, branch="k = 32"),
    Scenario("boxes3_rg1_w2", boxes3, 2, "contiguous", 250.0, rg_mode=1, components=3, branch="rg_mode 1 is run as 0"),
    Scenario("boxes3_interleaved_w4", boxes3, 4, "interleaved", 250.0, components=3,
             branch="more ranks than components: a rank grows nothing"),
    Scenario("boxes6_random_w4", boxes6, 4, "random", 250.0, components=6, branch="shares that are no index ranges"),
    Scenario("boxes3_rank1_nothing_w3", boxes3, 3, "rank1_nothing", 250.0, components=3, branch="m == 0 on one rank"),
    Scenario("boxes3_rank0_everything_w2", boxes3, 2, "rank0_everything", 250.0, components=3, branch="m == 0, one rank holds all"),
    Scenario("disc_retry1_w3", disc_sheet, 3, "interleaved", 50.0, retries=1,
             branch="one halo doubling; one component across every slab"),
    Scenario("disc_lattice_retry4_w2", disc_and_lattice400, 2, "random", 50.0, retries=4, branch="four halo doublings"),
    Scenario("coarse_lattice_uncertified_w2", coarse_lattice, 2, "contiguous", 50.0, retries=None,
             branch="more than six doublings: BS_ERR_UNCERTIFIED"),
    Scenario("far_boxes_w2", far_boxes, 2, "contiguous", 250.0, components=2, shift=1, branch="extent >= 2^21: shift 1"),
    Scenario("far_boxes_domain_edge_w3", far_boxes_at_domain_edge, 3, "interleaved", 250.0, components=2, shift=1,
             branch="shift 1 with the maximum at 2^23 - 2"),
    Scenario("far_boxes_negative_w2", far_boxes_negative, 2, "random", 250.0, components=2, shift=1,
             branch="shift 1 with negative coordinates"),
    Scenario("tiny40_w3", tiny40, 3, "interleaved", 0.0, retries=3, branch="slab + halo < k"),
    Scenario("lattice24_ties_w3", lattice24, 3, "contiguous", 0.0, branch="ties broken by global index across slab borders"),
    Scenario("walls_6k_w4", walls_6k, 4, "random", 250.0, branch="a single-component surface: three ranks grow nothing"),
    Scenario("plane_cube_12k_w4", plane_cube_12k, 4, "contiguous", 250.0, components=2, retries=1,
             branch="golden cloud, two components on four ranks"),
]
BY_NAME = {s.name: s for s in SCENARIOS}


# ---- the orchestration's own rules, restated -------------------------------------------------------------------
def start_halo(halo, radius=RADIUS):
    """h0 of sharded_impl (and of dist.segment_sharded_dev): max(halo > 0 ? halo : 2 * radius, radius)"""
    return max(halo if halo > 0 else 2.0 * radius, radius)


def expected_retries(max_kth, h0, limit=6):
    """smallest j with max_kth < h0 * 2^j (every point within h of a slab's points is present: the voxel edge is
    max(ceil(h), 500) >= h); None if j > limit"""
    j = 0
    while not max_kth < h0 * 2.0 ** j:
        j += 1
        if j > limit:
            return None
    return j


def retry_margin(max_kth, h0, limit=6):
    """distance in mm of max_kth from the nearest threshold h0 * 2^j"""
    return min(abs(max_kth - h0 * 2.0 ** j) for j in range(limit + 1))


def expected_shift(xyz):
    """the loop of sharded_impl: the largest extent over the axes, shifted down until it fits 21 bits"""
    x = np.asarray(xyz).astype(np.int64)
    ext = int((x.max(0) - x.min(0)).max())
    shift = 0
    while (ext >> shift) >= (1 << 21):
        shift += 1
    return shift


def morton_keys(xyz, origin, shift):
    """morton_key_kernel: bit b of (x, y, z) - origin >> shift at bit 3b + (0, 1, 2)"""
    v = (np.asarray(xyz).astype(np.int64) - np.asarray(origin, dtype=np.int64)) >> shift
    assert v.min() >= 0 and v.max() < (1 << 21)
    v = v.astype(np.uint64)
    key = np.zeros(len(v), np.uint64)
    for b in range(21):
        for a in range(3):
            key |= ((v[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + a)
    return key


def expected_slabs(xyz, parts, samples=1024):
    """Stage 1 of sharded_impl restated: every rank samples its sorted keys at `samples` evenly spaced positions (a rank
    without input contributes none), the splitters are the r/world quantiles of all samples, a point goes to the first
    rank whose splitter is >= its key.  -> list of arrays: the global indices of every rank's Morton slab (sorted)"""
    world = len(parts)
    xyz = np.asarray(xyz)
    keys = morton_keys(xyz, xyz.astype(np.int64).min(0), expected_shift(xyz))
    samp = []
    for p in parts:
        m = len(p)
        if m:
            sk = np.sort(keys[p])
            samp.append(sk[(np.arange(samples, dtype=np.int64) * (m - 1)) // (samples - 1)])
    samp = np.sort(np.concatenate(samp))
    valid = len(samp)
    spl = [samp[min(valid - 1, max(0, valid * r // world))] for r in range(1, world)]
    dest = np.searchsorted(np.array(spl, dtype=np.uint64), keys, side="left")  # first splitter >= key
    return [np.flatnonzero(dest == r) for r in range(world)]


def expected_deal(comp, slabs):
    """Stages 4-5 restated: every rank reports (root, points of it in my slab) of the components it holds part of, and
    dist.assign_components (the algorithm csrc/bs_sharded.hip restates) deals them.  comp [n]: component label of every
    point.  -> (rank that grows each point [n], n_grow per rank)"""
    from buildingsegment_amd import dist as bsd
    world = len(slabs)
    comp = np.asarray(comp)
    n = len(comp)
    root_of = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(root_of, comp, np.arange(n))  # the root is the smallest global index of the component
    roots, counts, ranks = [], [], []
    for r, s in enumerate(slabs):
        u, c = np.unique(root_of[comp[s]], return_counts=True)
        roots += u.tolist()
        counts += c.tolist()
        ranks += [r] * len(u)
    uniq, dest = bsd.assign_components(np.array(roots), np.array(counts), np.array(ranks), world)
    grower = dest[np.searchsorted(uniq, root_of[comp])]
    return grower, np.bincount(grower, minlength=world).tolist()


# ---- the facts of a scenario, computed once ------------------------------------------------------------------------
_CLOUDS = {}
_FACTS = {}


def cloud(sc):
    if sc.cloud not in _CLOUDS:
        xyz = np.ascontiguousarray(sc.cloud(), dtype=np.int32)
        xyz.setflags(write=False)
        _CLOUDS[sc.cloud] = xyz
    return _CLOUDS[sc.cloud]


def facts(oracle, sc):
    """-> dict: xyz, neigh, normals, labels, planes (the oracle's), kth [n] (float mm), max_kth, components, comp [n]
    (component label of every point, scipy), h0, retries, halo_mm.  The oracle's growth is skipped for the scenario
    that is expected to fail.  Cached per (cloud, k): the result is shared and must not be written to."""
    key = (sc.cloud, sc.k)
    if key not in _FACTS:
        import scipy.sparse as sp
        import scipy.sparse.csgraph as cg
        xyz = cloud(sc)
        n, k = len(xyz), sc.k
        ng, nr = oracle.knn_normals(xyz, k=k)
        d = xyz[ng[:, -1]].astype(np.int64) - xyz
        kth = np.sqrt((d * d).sum(1).astype(np.float64))
        A = sp.coo_matrix((np.ones(ng.size), (np.repeat(np.arange(n), k), ng.ravel())), shape=(n, n))
        ncomp, comp = cg.connected_components(A, directed=False)
        f = {"xyz": xyz, "neigh": ng, "normals": nr, "kth": kth, "max_kth": float(kth.max()), "components": int(ncomp),
             "comp": comp, "labels": None, "planes": None}
        if sc.retries is not None:
            f["labels"], f["planes"] = oracle.region_grow(xyz, nr, ng)
        for v in f.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _FACTS[key] = f
    f = dict(_FACTS[key])
    f["h0"] = start_halo(sc.halo)
    f["retries"] = expected_retries(f["max_kth"], f["h0"])
    f["halo_mm"] = None if f["retries"] is None else f["h0"] * 2.0 ** f["retries"]
    return f
