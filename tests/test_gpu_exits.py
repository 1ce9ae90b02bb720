"""The traversal's three exact exits on the GPU, table by table and ray by ray.

Tables: what k_world_top, k_column_top, k_dtop and k_horizon leave on the device (rv_world_export's
RV_WORLD_COLTOP / HORIZON / DTOP, rv_world_top_info) against the numpy references of tests/np_exits.py
-- which tests/test_exits_ref.py proves on the CPU -- after a bits import, a second import, each
rv_config.exits_off setting and each rv_world_edit: never too eager (below the safety bound), never too
timid (left at its "off" fill, stale, above the tightness bound).

Rays: every traversal the frame kernels instantiate (rv_trace_rays_variant: look-ahead 1 / 4 / 8, the sky
exit, trace_sun, the column skip) against the oracle's full march, bit for bit; the plain variants keep the
reference's step counts, the exits only shorten them; the column skip gives each ray the same result
whoever shares its wave."""
import numpy as np
import pytest

from gpu_world import rv, sun, tables
import np_exits as E

pytestmark = pytest.mark.gpu

HIT_FIELDS = ("pos", "normal", "u", "v")
COUNTS = (("sphere_steps", "n_sphere"), ("dda_steps", "n_dda"), ("csdf_checks", "n_check"))


def _context(rv, lg, vox, csdf=False, **kw):
    r = rv.StateRender(lg, 64, 64, **kw)
    r.world_import(rv.RV_WORLD_BITS, E.bits_of(vox))
    if csdf:
        r.csdf_build()
    return r


# ---------------------------------------------------------------- tables
@pytest.mark.parametrize("name", list(E.WORLDS))
def test_tables_equal_the_reference(rv, oracle, sun, name):
    lg, make = E.WORLDS[name]
    vox = make(oracle)
    r = _context(rv, lg, vox)
    try:
        yt, ct, hz, dt = tables(rv, r)
    finally:
        r.close()
    slack = E.check_tables(E.reference(vox, sun, name), yt, ct, hz, dt, name)
    print(f"{name} {vox.shape[::-1]}: ytop {yt}, {ct.size} coltop and {hz.size} horizon cells, {dt.size} dtop cells "
          f"compared; horizon - safety {slack[0]}, tightness - horizon {slack[1]}")


def test_exits_off_gives_the_documented_fills(rv, oracle, sun):
    """rv_config.exits_off: SKY drops all three exits (ytop = Y, both tables at their fills, no column tops:
    the export gives zeros), COLUMN only the dtop table, SUN only the horizon; what stays on is built."""
    name = "terrain_6_7_5"
    lg, make = E.WORLDS[name]
    vox = make(oracle)
    ref = E.reference(vox, sun, name)
    assert ref["ytop"] < vox.shape[1]
    for off in (rv.RV_EXIT_SKY, rv.RV_EXIT_COLUMN, rv.RV_EXIT_SUN, rv.RV_EXIT_COLUMN | rv.RV_EXIT_SUN):
        r = _context(rv, lg, vox, exits_off=off)
        try:
            yt, ct, hz, dt = tables(rv, r)
        finally:
            r.close()
        if off & rv.RV_EXIT_SKY:
            assert yt == vox.shape[1] and not ct.any()
        else:
            assert yt == ref["ytop"] and np.array_equal(ct, ref["coltop"])
        if off & (rv.RV_EXIT_SKY | rv.RV_EXIT_SUN):
            assert (hz == E.HORIZON_OFF).all(), off
        else:
            E.check_tables(ref, yt, ct, hz, ref["dtop"], f"exits_off={off}")
        if off & (rv.RV_EXIT_SKY | rv.RV_EXIT_COLUMN):
            assert (dt == E.DTOP_OFF).all(), off
        else:
            assert np.array_equal(dt, ref["dtop"]), off


def test_tables_follow_a_second_import(rv, oracle, sun):
    """rv_world_import(BITS) of other bits into the same context, a lower world after a higher one (the column
    tops are atomic maxima: a table not cleared first would keep the old peaks) and an empty one last."""
    lg = (6, 6, 5)
    worlds = [("sparse", E.WORLDS["sparse"][1](oracle))]
    low = worlds[0][1].copy()
    low[:, 20:, :] = False
    low[:16, 9:, :] = False
    worlds += [("sparse, lowered", low), ("no voxel", np.zeros_like(low))]
    assert E.WORLDS["sparse"][0] == lg and E.ytop(low) < E.ytop(worlds[0][1])
    r = rv.StateRender(lg, 64, 64)
    try:
        for what, vox in worlds:
            r.world_import(rv.RV_WORLD_BITS, E.bits_of(vox))
            E.check_tables(E.reference(vox, sun), *tables(rv, r), what)
    finally:
        r.close()


def test_tables_follow_each_edit(rv, oracle, sun):
    """rv_world_edit on its local path (rv_world_edit_info: not the whole-grid build): after each edit the
    bits are the edited bits and every table equals the reference for them -- none stale, none at "off"."""
    lg, make = E.EDIT_WORLD
    vox = make(oracle)
    r = _context(rv, lg, vox, csdf=True)
    try:
        E.check_tables(E.reference(vox, sun, "edit0"), *tables(rv, r), "before the edits")
        for n, (what, boxes) in enumerate(E.edit_steps(vox), 1):
            r.world_edit(boxes)
            edits, cells, full = r.world_edit_info()
            assert edits == n and cells > 0 and not full, (what, edits, cells, full)
            vox = E.apply_boxes(vox, boxes)
            assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), E.bits_of(vox)), what
            slack = E.check_tables(E.reference(vox, sun, f"edit{n}"), *tables(rv, r), what)
            print(f"{what} {boxes}: local, slack {slack}")
    finally:
        r.close()


# ---------------------------------------------------------------- rays
RAY_WORLDS = {"terrain128_cut90": E.WORLDS["terrain128_cut90"], "terrain_8_6_7_cut56": E.EDIT_WORLD}
_RAY = {}


@pytest.fixture(scope="module")
def ray_world(rv, oracle, sun):
    """Factory: (context, oracle world, voxels, ray sets with the oracle's results) per ray world; the
    contexts live until the module ends, the references are computed once and never changed."""
    def make(name):
        if name not in _RAY:
            lg, mk = RAY_WORLDS[name]
            vox = mk(oracle)
            ow = oracle.OracleWorld(*lg)
            ow.bits[:] = E.bits_of(vox)
            ow.build_csdf()
            r = _context(rv, lg, vox, csdf=True)
            assert np.array_equal(r.world_export(rv.RV_WORLD_CSDF), ow.csdf)
            rays = {"sky": E.sky_rays((ow.X, ow.Y, ow.Z)), "sun": E.sun_rays(ow, sun), "col": E.column_rays(vox)[:3]}
            _RAY[name] = (r, ow, vox, {k: (v, ow.trace_batch(*v)) for k, v in rays.items()})
        return _RAY[name]
    yield make
    for r, *_ in _RAY.values():
        r.close()
    _RAY.clear()


def _same_hits(g, o, what):
    assert np.array_equal(g["hit"], o["hit"]) and np.array_equal(g["undef"], o["undef"]), what
    for f in HIT_FIELDS:
        assert np.array_equal(g[f].view(np.uint32), o[f].view(np.uint32)), (what, f)


@pytest.mark.parametrize("g", [1, 4, 8])
@pytest.mark.parametrize("world", list(RAY_WORLDS))
def test_plain_variants_keep_the_references_step_counts(rv, ray_world, world, g):
    """No SKY, SUN or COL: look-ahead 1, 4 and 8 (stop search + re-walk) give the oracle's hit record and its
    sphere, DDA and check counts for every ray -- on all three ray sets."""
    r, ow, vox, rays = ray_world(world)
    for kind, (ray, o) in rays.items():
        got = r.trace_rays(*ray, variant=g)
        assert len(got) % 64 != 0
        _same_hits(got, o, (world, g, kind))
        for a, b in COUNTS:
            assert np.array_equal(got[a], o[b]), (world, g, kind, a)
        assert not got["pad"].any()
        print(f"{world} look-ahead {g} {kind}: {len(got)} rays equal the oracle, counts included")


@pytest.mark.parametrize("g", [1, 4, 8])
@pytest.mark.parametrize("world", list(RAY_WORLDS))
def test_sky_exit_keeps_every_hit(rv, ray_world, world, g):
    r, ow, vox, rays = ray_world(world)
    ray, o = rays["sky"]
    got = r.trace_rays(*ray, variant=g | rv.RV_TRACE_SKY)
    _same_hits(got, o, (world, g))
    assert (got["sphere_steps"] <= o["n_sphere"]).all()
    print(f"{world} look-ahead {g} | SKY: {len(got)} rays, sphere steps {got['sphere_steps'].sum()} of the "
          f"oracle's {o['n_sphere'].sum()}, hit share {o['hit'].mean():.2f}")
    assert got["sphere_steps"].sum() < o["n_sphere"].sum()      # the exit does cut the march
    assert 0.1 < o["hit"].mean() < 0.9


@pytest.mark.parametrize("sky", [True, False], ids=["sky", "nosky"])
@pytest.mark.parametrize("g", [1, 4, 8])
@pytest.mark.parametrize("world", list(RAY_WORLDS))
def test_sun_exit_keeps_every_shadow_hit(rv, ray_world, world, g, sky):
    r, ow, vox, rays = ray_world(world)
    ray, o = rays["sun"]
    got = r.trace_rays(*ray, variant=g | rv.RV_TRACE_SUN | (rv.RV_TRACE_SKY if sky else 0))
    _same_hits(got, o, (world, g, sky))
    assert (got["sphere_steps"] <= o["n_sphere"]).all()
    print(f"{world} look-ahead {g} | SUN{' | SKY' if sky else ''}: {len(got)} rays, sphere steps "
          f"{got['sphere_steps'].sum()} of the oracle's {o['n_sphere'].sum()}, hit share {o['hit'].mean():.2f}")
    assert got["sphere_steps"].sum() < o["n_sphere"].sum()      # the horizon does cut the march
    assert 0.1 < o["hit"].mean() < 0.9                          # shadowed and lit points both


@pytest.mark.parametrize("sky", [True, False], ids=["sky", "nosky"])
@pytest.mark.parametrize("g", [4, 8])
@pytest.mark.parametrize("world", list(RAY_WORLDS))
def test_column_skip_keeps_every_hit(rv, ray_world, world, g, sky):
    """COL against the same traversal without it -- every field, the DDA and check counts too -- and against
    the oracle; the skip fires on more than 5 % of the groups and on both branches of the iy - G row bound."""
    r, ow, vox, rays = ray_world(world)
    ray, o = rays["col"]
    base = g | (rv.RV_TRACE_SKY if sky else 0)
    a, b = r.trace_rays(*ray, variant=base | rv.RV_TRACE_COL), r.trace_rays(*ray, variant=base)
    for f in a.dtype.names:
        if f != "pad":
            assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), (world, g, sky, f)
    _same_hits(a, o, (world, g, sky))
    assert (a["sphere_steps"] <= o["n_sphere"]).all()
    if not sky:
        for p, q in COUNTS:
            assert np.array_equal(a[p], o[q]), (world, g, p)
    groups = E.groups_walked(a["dda_steps"], g)
    print(f"{world} look-ahead {g} | COL{' | SKY' if sky else ''}: {len(a)} rays, {a['pad'].sum()} of "
          f"{groups.sum()} groups skipped, hit share {o['hit'].mean():.2f}")
    assert not b["pad"].any() and a["pad"].sum() > 0.05 * groups.sum()
    desc = ray[1][:, 1] < 0
    assert a["pad"][desc].sum() > 0 and a["pad"][~desc].sum() > 0
    assert 0.1 < o["hit"].mean() < 0.9


def test_unknown_variants_are_refused(rv, ray_world):
    r, ow, vox, rays = ray_world("terrain128_cut90")
    ray = tuple(v[:10] for v in rays["sky"][0])
    T = rv
    for v in (0, 2, 3, 16, 0x800 | 4, 1 | T.RV_TRACE_COL, 4 | T.RV_TRACE_COL | T.RV_TRACE_SUN,
              8 | T.RV_TRACE_SKY | T.RV_TRACE_COL | T.RV_TRACE_SUN, -1):
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            r.trace_rays(*ray, variant=v)
    assert len(r.trace_rays(*(v[:0] for v in ray), variant=4)) == 0


@pytest.mark.parametrize("g", [4, 8])
def test_a_rays_result_does_not_depend_on_its_wave_mates(rv, ray_world, g):
    """wave_all(skip) decides per wave whether a group's voxel gathers are issued.  The column-skip rays in
    three orders -- sorted by height above the local top (whole waves skip, whole waves do not), shuffled
    (every wave mixed), and each skimming ray next to one that dives into the terrain -- give every ray the
    same record, its skipped-group count included, and the record of the run without COL."""
    world = "terrain128_cut90"
    r, ow, vox, rays = ray_world(world)
    (org, d, dist), o = rays["col"]
    n = len(dist)
    height = E.column_rays(vox)[3]
    var = g | rv.RV_TRACE_SKY
    plain = r.trace_rays(org, d, dist, variant=var)
    rng = np.random.default_rng(5)
    dive = np.stack([d[:, 0], -np.float32(3.0) * np.hypot(d[:, 0], d[:, 2]) - np.float32(0.1), d[:, 2]], 1)
    dive = (dive / np.linalg.norm(dive, axis=1, keepdims=True)).astype(np.float32)
    runs = {}
    for what, perm in (("sorted", np.argsort(height, kind="stable")), ("shuffled", rng.permutation(n))):
        got = r.trace_rays(org[perm], d[perm], dist[perm], variant=var | rv.RV_TRACE_COL)
        back = np.empty_like(got)
        back[perm] = got
        runs[what] = back
    o2, d2 = np.repeat(org, 2, axis=0), np.repeat(d, 2, axis=0)
    d2[1::2] = dive
    got = r.trace_rays(o2, d2, np.zeros(2 * n, np.float32), variant=var | rv.RV_TRACE_COL)
    runs["interleaved"] = got[0::2]
    _same_hits(got[1::2], ow.trace_batch(org, dive, dist), "the diving rays")
    assert got[1::2]["hit"].mean() > 0.9
    for what, back in runs.items():
        for f in back.dtype.names:
            ref = runs["sorted"] if f == "pad" else plain
            assert np.array_equal(back[f].view(np.uint32), ref[f].view(np.uint32)), (what, f)
        assert back["pad"].sum() > 0, what
    _same_hits(plain, o, "without COL")
    print(f"look-ahead {g}: {n} rays in 3 orders, {runs['sorted']['pad'].sum()} skipped groups each")


def test_exit_variants_follow_a_pillar_edit(rv, oracle, sun, ray_world):
    """A pillar raised by rv_world_edit into the skimming rays' path: the COL and SUN variants equal the
    oracle on the edited bits (a stale dtop or horizon would let rays pass through the pillar)."""
    lg, make = E.EDIT_WORLD
    vox = make(oracle)
    _, ow0, _, rays = ray_world("terrain_8_6_7_cut56")
    boxes = E.pillar_boxes(vox)
    ow = oracle.OracleWorld(*lg)
    ow.bits[:] = E.bits_of(E.apply_boxes(vox, boxes))
    ow.build_csdf()
    r = _context(rv, lg, vox, csdf=True)
    try:
        r.world_edit(boxes)
        assert r.world_edit_info()[0] == 1 and not r.world_edit_info()[2]
        assert np.array_equal(r.world_export(rv.RV_WORLD_CSDF), ow.csdf)
        E.check_tables(E.reference(E.apply_boxes(vox, boxes), sun, "pillar"), *tables(rv, r), "pillar")
        for kind, flags in (("col", rv.RV_TRACE_COL), ("sun", rv.RV_TRACE_SUN)):
            ray, before = rays[kind]
            o = ow.trace_batch(*ray)
            changed = int((o["pos"].view(np.uint32) != before["pos"].view(np.uint32)).any(axis=1).sum())
            assert changed >= 10, (kind, changed)
            for g in (4, 8):
                got = r.trace_rays(*ray, variant=g | rv.RV_TRACE_SKY | flags)
                _same_hits(got, o, (kind, g))
                assert (got["sphere_steps"] <= o["n_sphere"]).all()
                if kind == "col":
                    plain = r.trace_rays(*ray, variant=g | rv.RV_TRACE_SKY)
                    assert got["pad"].sum() > 0 and not plain["pad"].any()
                    for f in ("sphere_steps", "dda_steps", "csdf_checks"):
                        assert np.array_equal(got[f], plain[f]), (g, f)
            print(f"pillar, {kind}: {len(o)} rays at look-ahead 4 and 8, {changed} of them changed by the edit")
    finally:
        r.close()
