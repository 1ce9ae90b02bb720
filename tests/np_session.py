"""A host model of the world window as include/rvgrt.h describes it, and seeded random sessions of world
calls to replay against it and against a context.  The model keeps the window's origin, dense voxels, the
persistence flag, dirty set and store, the texture origin and follow flag, the GI grid as the world calls
move it, and the counters the *_info calls report.  It knows nothing of kept work, local rebuilds or
scratch: the CSDF, the exit tables and column bits are derived from the voxels when somebody asks.  It
holds no GPU call; every rule is restated from the header's text.

A session is a list of plain tuples ("scroll", 16, -8), ("edit", ((x0, y0, z0, x1, y1, z1, solid), ...)), ...
that `Session.apply` understands; `ops` draws one from a seed, `replay` runs a list literally."""
import numpy as np

from gpu_world import dims, gi_dims, pack, voxels
import np_world as R

ORIGIN = (40, -24)   # not a multiple of any window size, one coordinate negative


def put_column(lg, k):
    """Column bits (2 Y uint32) that no generator makes, drawn from the integer k: solid below a height with
    holes in it, and a slab floating above."""
    Y = 1 << lg[1]
    rng = np.random.default_rng(1000 + k)
    col = np.zeros((8, Y, 8), bool)     # [z, y, x]: bit x | y << 3 | z << (3 + log2_y)
    h = int(rng.integers(Y // 4, 3 * Y // 4))
    col[:, :h, :] = rng.uniform(size=(8, h, 8)) > 0.1
    col[2:6, h + 3:h + 5, 1:7] = True
    return np.packbits(col.ravel(), bitorder="little").view(np.uint32)


def relight_box(lg, boxes, margin=0):
    """rv_gi_relight_box restated: the GI-cell bounding box of the boxes' voxels (cell = voxel >> 2), grown
    by margin cells and clipped to the grid."""
    G = gi_dims(lg)
    lo = [max(0, (min(b[a] for b in boxes) >> 2) - margin) for a in range(3)]
    hi = [min(G[a], ((max(b[3 + a] for b in boxes) - 1) >> 2) + 1 + margin) for a in range(3)]
    return tuple(lo + hi)


def edit_region(lg, boxes):
    """rv_world_edit_region restated: the boxes' coarse bounding box grown by 64 cells, clipped; its volume."""
    S = [1 << (l - 1) for l in lg]
    r = []
    for a in range(3):
        r += [max(0, (min(b[a] for b in boxes) >> 1) - 64), min(S[a], ((max(b[3 + a] for b in boxes) - 1) >> 1) + 65)]
    return tuple(r), (r[1] - r[0]) * (r[3] - r[2]) * (r[5] - r[4])


_SLABS = {}


def generated_planes(oracle, lg, origin, axis, lo, n):
    """Voxels [z, y, x] of the n planes from plane `lo` along axis (0 = x, 2 = z) of the generated window at
    `origin`.  The terrain is a function of terrain coordinates alone, so the planes are generated as a
    narrow window of their own, once per place (np_world.terrain keeps whole windows the same way)."""
    key = (lg, origin, axis, lo, n)
    if key not in _SLABS:
        l = max(3, int(n - 1).bit_length())
        if axis == 0:
            v = oracle.OracleWorld(l, lg[1], lg[2], ox=origin[0] + lo, oz=origin[1]).fill().voxels()[:, :, :n]
        else:
            v = oracle.OracleWorld(lg[0], lg[1], l, ox=origin[0], oz=origin[1] + lo).fill().voxels()[:n]
        _SLABS[key] = v
    return _SLABS[key]


class Session:
    """The window after rv_world_build at `origin`.  gi=False: no GI grid (the generator's and the CPU tests'
    cheap form).  `log` receives (call index, what, key) for the things a trace is chosen to contain."""

    def __init__(self, oracle, lg, origin=ORIGIN, atlas=None, gi=True, saturate=False):
        # a region that is the whole grid is a whole-grid build and the other way round only while at most
        # one axis is longer than 128 voxels: then the nested input boxes of the local passes cover the grid
        # in every pass exactly when the innermost does (rv_world_edit_info's last_full below)
        assert sorted(lg)[1] <= 7, "the model's last_full holds for worlds with one long axis at the most"
        self.O, self.lg, self.atlas, self.saturate = oracle, tuple(lg), atlas, saturate
        self.origin = (int(origin[0]), int(origin[1]))
        self.persist_on, self.dirty, self.store, self.tag = False, set(), {}, {}
        self.tex, self.follow = (0, 0), False
        self.edits, self.edit_cells, self.edit_full = 0, 0, False
        self.scrolls, self.scroll_cells, self.scroll_full = 0, 0, False
        self.captured = self.restored = self.restored_in_build = 0
        self.relights = (0, 0, 0)
        self.bodies = (0, 0)
        self.calls, self.log = 0, []
        self.steps = []                  # (axis, d, full) of every scroll step, for the coverage checks
        self._restored_once, self._edited_since = set(), set()
        self.gi = None
        self.vox = R.terrain(oracle, self.lg, *self.origin).copy()
        if gi:
            self.gi = self._gi_init()

    # ------------------------------------------------------------ derived on demand
    def bits(self):
        return pack(self.vox)

    def oracle_world(self, csdf=True):
        ow = self.O.OracleWorld(*self.lg, atlas=self.atlas)
        ow.bits[:] = self.bits()
        if csdf:
            ow.build_csdf()
        if self.gi is not None:
            ow.gi[:] = self.gi.view(np.uint8)
        return ow

    def csdf(self):
        return self.oracle_world().csdf

    def column_bits(self, bx, bz):
        return R.column_bits(self.vox, bx, bz)

    def key(self, bx, bz):
        return (self.origin[0] + 8 * bx, self.origin[1] + 8 * bz)

    def column_of(self, key):
        """(bx, bz) of a key's column in the window, or None."""
        X, _, Z = dims(self.lg)
        rx, rz = key[0] - self.origin[0], key[1] - self.origin[1]
        if rx % 8 or rz % 8 or not (0 <= rx < X and 0 <= rz < Z):
            return None
        return rx // 8, rz // 8

    def dirty_columns(self):
        """The dirty keys that are columns of the window, as (bx, bz)."""
        return sorted(c for c in (self.column_of(k) for k in self.dirty) if c is not None)

    def persist_info(self):
        Y = dims(self.lg)[1]
        return {"on": self.persist_on, "dirty_columns": len(self.dirty), "stored_columns": len(self.store),
                "stored_bytes": len(self.store) * 8 * Y, "captured_total": self.captured,
                "restored_total": self.restored}

    def store_list(self):
        return sorted(self.store, key=lambda k: (k[1], k[0]))

    def edit_info(self):
        return self.edits, self.edit_cells, self.edit_full

    def scroll_info(self):
        return self.scrolls, self.scroll_cells, self.scroll_full, self.origin

    def _gi_init(self):
        ow = self.oracle_world()
        ow.gi_init(saturate=self.saturate)
        return ow.gi.view(np.uint32).copy()

    # ------------------------------------------------------------ persistence
    def _capture(self, key, col):
        if key in self.store:
            self.log.append((self.calls, "replaced", key))
            if self.tag[key] == "put":
                self.log.append((self.calls, "put_overwritten", key))
        self.store[key] = self.column_bits(*col).copy()
        self.tag[key] = "captured"
        self.captured += 1
        self.log.append((self.calls, "capture", key))

    def _restore(self, cols):
        """The stored keys among these columns of the window take their stored bits."""
        for bx, bz in cols:
            key = self.key(bx, bz)
            if key not in self.store:
                continue
            Y = dims(self.lg)[1]
            col = np.unpackbits(self.store.pop(key).view(np.uint8), bitorder="little").reshape(8, Y, 8)
            self.vox[8 * bz:8 * bz + 8, :, 8 * bx:8 * bx + 8] = col.astype(bool)
            self.dirty.add(key)
            self.restored += 1
            self.log.append((self.calls, "restore", key))
            if self.tag.pop(key) == "put":
                self.log.append((self.calls, "put_consumed", key))
            if key in self._edited_since:
                self.log.append((self.calls, "restore_after_reedit", key))
                self._edited_since.discard(key)
            self._restored_once.add(key)

    def _mark(self, cols):
        for bx, bz in cols:
            key = self.key(bx, bz)
            self.dirty.add(key)
            if key in self._restored_once:
                self._edited_since.add(key)

    def _window_columns(self):
        X, _, Z = dims(self.lg)
        return [(bx, bz) for bz in range(Z // 8) for bx in range(X // 8)]

    # ------------------------------------------------------------ the calls
    def build(self):
        self.vox = R.terrain(self.O, self.lg, *self.origin).copy()
        before = self.restored
        if self.persist_on:
            self.dirty.clear()
            self._restore(self._window_columns())
        self.restored_in_build = self.restored - before
        if self.gi is not None:
            self.gi = self._gi_init()

    def import_bits(self, bits):
        self.vox = voxels(np.asarray(bits, np.uint32), self.lg).copy()
        if self.persist_on:
            self._mark(self._window_columns())

    def edit(self, boxes):
        if not boxes:
            return
        before = self.vox.copy()
        for (x0, y0, z0, x1, y1, z1, s) in boxes:
            self.vox[z0:z1, y0:y1, x0:x1] = bool(s)
        if np.array_equal(before, self.vox):
            self.edit_cells, self.edit_full = 0, False
            self.log.append((self.calls, "noop_edit", None))
            return
        if self.persist_on:
            for b in boxes:
                self._mark([(bx, bz) for bz in range(b[2] >> 3, ((b[5] - 1) >> 3) + 1)
                            for bx in range(b[0] >> 3, ((b[3] - 1) >> 3) + 1)])
        region, cells = edit_region(self.lg, boxes)
        S = [1 << (l - 1) for l in self.lg]
        self.edits += 1
        self.edit_cells, self.edit_full = cells, region == (0, S[0], 0, S[1], 0, S[2])
        self.log.append((self.calls, "edit_full" if self.edit_full else "edit_local", None))

    def _step(self, axis, d):
        X, Y, Z = dims(self.lg)
        dim = X if axis == 0 else Z
        nb, ab, ax = dim // 8, min(abs(d), dim) // 8, 2 - axis
        cols = self._window_columns()
        leave = range(0, ab) if d > 0 else range(nb - ab, nb)
        enter = range(nb - ab, nb) if d > 0 else range(0, ab)
        if self.persist_on:
            for c in cols:
                if c[axis // 2] in leave and self.key(*c) in self.dirty:
                    self._capture(self.key(*c), c)
                    self.dirty.discard(self.key(*c))
        self.origin = (self.origin[0] + (d if axis == 0 else 0), self.origin[1] + (d if axis == 2 else 0))
        sl = [slice(None)] * 3
        if abs(d) >= dim:
            self.vox = R.terrain(self.O, self.lg, *self.origin).copy()
        else:
            self.vox = np.roll(self.vox, -d, axis=ax)
            lo = dim - d if d > 0 else 0
            sl[ax] = slice(lo, lo + abs(d))
            self.vox[tuple(sl)] = generated_planes(self.O, self.lg, self.origin, axis, lo, abs(d))
        if self.persist_on:
            self._restore([c for c in cols if c[axis // 2] in enter])
        if self.gi is not None:
            G = gi_dims(self.lg)
            init = self._gi_init().reshape(G[::-1])     # gi_init in the step's new world
            if abs(d) >= dim:
                g = init
            else:
                g = np.roll(self.gi.reshape(G[::-1]), -d // 4, axis=ax)
                sl[ax] = slice((dim - d) // 4, dim // 4) if d > 0 else slice(0, -d // 4)
                g[tuple(sl)] = init[tuple(sl)]
            self.gi = np.ascontiguousarray(g).ravel()
        _, _, cells, full = R.expected_plan(self.lg, axis, d)
        self.steps.append((axis, d, full))
        return cells, full

    def scroll(self, dx, dz):
        assert dx % 8 == 0 and dz % 8 == 0
        if dx == 0 and dz == 0:
            return
        cells, full = 0, False
        for axis, d in ((0, dx), (2, dz)):
            if d:
                c, f = self._step(axis, d)
                cells, full = cells + c, full or f
        self.scrolls += 1
        self.scroll_cells, self.scroll_full = cells, full
        if self.follow:
            self.tex = (self.tex[0] + dx, self.tex[1] + dz)
        if dx and dz:
            self.log.append((self.calls, "diagonal", None))
        X, _, Z = dims(self.lg)
        if abs(dx) >= X or abs(dz) >= Z:
            self.log.append((self.calls, "emptied", None))

    def persist(self, on):
        self.persist_on = bool(on)

    def flush(self):
        if self.persist_on:
            for c in self.dirty_columns():
                self._capture(self.key(*c), c)

    def store_put(self, wx, wz, bits):
        if (wx - self.origin[0]) % 8 or (wz - self.origin[1]) % 8:
            raise ValueError("RV_ERR_INVALID: no column can have this key")
        if len(bits) != 2 * dims(self.lg)[1]:
            raise ValueError("RV_ERR_INVALID: a column is 8 Y bytes")
        where = "put_outside" if self.column_of((wx, wz)) is None else \
            "put_dirty" if (wx, wz) in self.dirty else "put_clean"
        self.log.append((self.calls, where, (wx, wz)))
        self.store[(wx, wz)] = np.array(bits, np.uint32)
        self.tag[(wx, wz)] = "put"

    def store_get(self, wx, wz):
        if (wx, wz) not in self.store:
            raise ValueError("RV_ERR_INVALID: not in the store")
        return self.store[(wx, wz)]

    def store_clear(self):
        self.store.clear()
        self.tag.clear()
        self.dirty.clear()

    def texture_origin_set(self, ox, oz):
        self.tex = (int(ox), int(oz))

    def texture_follow_scroll(self, on):
        self.follow = bool(on)

    def relight(self, box, frame0, iterations, init):
        """np_world.expect_relight on the model's grid; the oracle has no texture origin."""
        if iterations == 0 and not init:
            return
        if self.gi is None:
            return self.count_relight(box, iterations)
        assert self.tex == (0, 0), "the oracle's relight samples textures at origin (0, 0)"
        ow = self.oracle_world()
        self.gi = R.expect_relight(ow, box, frame0, iterations, init=init, saturate=self.saturate)
        self.count_relight(box, iterations)

    def count_relight(self, box, iterations):
        cells = (box[3] - box[0]) * (box[4] - box[1]) * (box[5] - box[2])
        n, c, r = self.relights
        self.relights = (n + 1, c + cells, r + cells * iterations)

    def apply(self, op):
        """One call of a trace.  The ops that stand for invalid calls and for frames leave the model alone."""
        name, a = op[0], op[1:]
        if name == "edit":
            self.edit(a[0])
        elif name == "store_put":
            self.store_put(a[0], a[1], put_column(self.lg, a[2]))
        elif name == "relight":
            self.relight(*a)
        elif name in ("bad_put", "bad_get", "bodies", "frames"):
            pass
        else:
            getattr(self, name)(*a)
        self.calls += 1
        return self


def replay(oracle, lg, trace, origin=ORIGIN, **kw):
    """The model after the calls of `trace`, run literally."""
    m = Session(oracle, lg, origin, **kw)
    for op in trace:
        m.apply(op)
    return m


def coverage(m):
    """How often a replayed model met each of the things the committed seeds are chosen for."""
    names = ("capture", "restore", "restore_after_reedit", "replaced", "noop_edit", "diagonal", "emptied",
             "put_consumed", "put_overwritten", "edit_local", "edit_full")
    c = {n: sum(1 for e in m.log if e[1] == n) for n in names}
    c["step_local"] = sum(1 for s in m.steps if not s[2])
    c["step_full"] = sum(1 for s in m.steps if s[2])
    return c


def kinds(m, trace):
    """The calls of MIX that a trace holds (m: the model after it), a relight with and without INIT apart;
    persist_toggle: persistence off, an edit or a scroll without it, and on again."""
    names = [op[0] for op in trace]
    k = set(names) & {"scroll", "flush", "store_clear", "texture_origin_set", "bodies", "bad_put", "bad_get"}
    k |= {e[1] for e in m.log} & {"noop_edit", "put_dirty", "put_clean", "put_outside"}
    k |= {"edit"} if m.edits else set()
    k |= {"follow_toggle"} if "texture_follow_scroll" in names else set()
    k |= {("relight_init" if op[4] else "relight") for op in trace if op[0] == "relight"}
    for i, op in enumerate(trace):
        if op == ("persist", 0) and ("persist", 1) in trace[i:]:
            j = i + trace[i:].index(("persist", 1))
            if {"edit", "scroll"} & set(names[i:j]):
                k.add("persist_toggle")
    return k


# ---------------------------------------------------------------- the generator
# weights of the calls drawn at random, next to the purposeful edits, scrolls and puts; a session's mix
# overrides them by name (0 leaves a call out)
MIX = {"scroll": 16, "edit": 16, "noop_edit": 3, "flush": 3, "put_dirty": 3, "put_clean": 3, "put_outside": 3,
       "store_clear": 1, "persist_toggle": 3, "texture_origin_set": 4, "follow_toggle": 4, "relight": 7,
       "bodies": 3, "bad_put": 1, "bad_get": 1}

# the committed sessions, (log2 dims, seed, calls): chosen on the CPU so that each meets every condition of
# tests/test_world_session.py; the GPU tests replay the same ones
ENDING = (("flush",), ("build",))
WORLD_SESSIONS = [((9, 7, 7), 3, 16), ((9, 7, 7), 9, 16), ((9, 7, 7), 11, 16), ((7, 7, 9), 8, 16), ((7, 7, 9), 14, 16),
                  ((7, 7, 9), 21, 16), ((7, 7, 7), 1, 16), ((7, 7, 7), 15, 16), ((7, 7, 7), 24, 16)]
# Traces written out by hand, replayed like the random ones on a (7, 7, 7) window (the form a failing random
# session is cut down to).  put_of_a_dirty_column: store_put of a key whose column is in the window and
# dirty -- replaced once when the column leaves, once by a flush -- and a restored column's exits after an
# edit since the last whole build.  persist_off_and_on: an edit and a scroll with persistence off mark and
# capture nothing and clear nothing -- the dirty key of a column that left uncaptured is still there when its
# terrain comes back, and is captured and restored as generated terrain later -- then store_get of a missing
# key, a relight with and without INIT, and a store_clear before the build, which forgets the edit made without
# persistence.
LITERAL_SESSIONS = {
    "put_of_a_dirty_column": [
        ("persist", 1), ("edit", ((2, 0, 18, 6, 128, 22, 0),)), ("store_put", 40, -8, 7), ("scroll", 16, 0),
        ("edit", ((60, 50, 60, 64, 90, 66, 1),)), ("scroll", -16, 0), ("edit", ((1, 40, 17, 7, 60, 23, 1),)),
        ("store_put", 40, -8, 8), ("store_put", 32, -8, 9), ("scroll", -8, 8), ("scroll", 8, -8), ("flush",),
        ("build",)],
    "persist_off_and_on": [
        ("persist", 1), ("edit", ((2, 0, 18, 6, 128, 22, 0),)), ("persist", 0),
        ("edit", ((42, 0, 43, 46, 128, 47, 0), (44, 100, 41, 50, 110, 45, 1))), ("scroll", 16, -8), ("persist", 1),
        ("scroll", -16, 8), ("bad_get", 40, -8), ("relight", (9, 0, 9, 14, 32, 13), 4000000000, 2, True),
        ("relight", (9, 0, 9, 14, 32, 13), 77, 1, False), ("bad_put", 44, -8), ("scroll", 24, 0), ("bodies", 5),
        ("scroll", -24, 0), ("flush",), ("store_clear",), ("build",)],
}
FRAME_MIX = {"store_clear": 0, "bad_put": 0, "bad_get": 0, "persist_toggle": 0, "texture_origin_set": 0,
             "follow_toggle": 0, "relight": 12, "bodies": 8}
ANCHORED_MIX = dict(FRAME_MIX, texture_origin_set=4, follow_toggle=2, relight_anchored=1)
FRAME_SESSIONS = {False: (12, 24), True: (11, 24)}      # anchored textures -> (seed, trace entries)
RANK_SESSION = (3, 24)


def _small_box(rng, m, where):
    """One box of at most 6 x 10 x 6 voxels: in a given brick column, straddling a brick-column border, at a
    face of the window or anywhere; half of them across the terrain's surface."""
    X, Y, Z = dims(m.lg)
    sx, sy, sz = (int(rng.integers(1, 7)), int(rng.integers(1, 11)), int(rng.integers(1, 7)))
    if isinstance(where, tuple):
        x0, z0 = 8 * where[0] + int(rng.integers(0, 8)), 8 * where[1] + int(rng.integers(0, 8))
    elif where == "border":
        x0, z0 = 8 * int(rng.integers(1, X // 8)) - 1 - int(rng.integers(0, sx)), \
            8 * int(rng.integers(1, Z // 8)) - 1 - int(rng.integers(0, sz))
    elif where == "face":
        x0, z0 = int(rng.integers(0, X - sx + 1)), int(rng.integers(0, Z - sz + 1))
        if rng.uniform() < 0.5:
            x0 = int(rng.choice([0, X - sx]))
        else:
            z0 = int(rng.choice([0, Z - sz]))
    else:
        x0, z0 = int(rng.integers(0, X - sx + 1)), int(rng.integers(0, Z - sz + 1))
    x0, z0 = min(max(x0, 0), X - sx), min(max(z0, 0), Z - sz)
    if rng.uniform() < 0.5:      # the rows around the surface of this voxel column
        col = m.vox[z0, :, x0]
        top = int(Y - np.argmax(col[::-1])) if col.any() else 0
        y0 = top - int(rng.integers(0, sy + 1))
    else:
        y0 = int(rng.integers(0, Y - sy + 1))
    y0 = min(max(y0, 0), Y - sy)
    return (x0, y0, z0, x0 + sx, y0 + sy, z0 + sz, int(rng.integers(0, 2)))


def ops(seed, lg, n, mix=None, oracle=None, origin=ORIGIN, purpose=0.6, ending=(), frames=False):
    """A session of n calls drawn from `seed`: ("persist", 1), then calls by the weights of MIX updated with
    `mix`, then `ending`.  Uniform calls mostly miss what the sessions are for, so the generator runs a model
    of its own and shapes them: scrolls go home about a third of the time, so that columns come back, or
    carry a dirty column out through its nearest face; edits favour a few columns near the home window's
    faces and columns that have been away and back; store_put chooses its keys by what the window holds at
    that call; and with probability `purpose` a call is the next step towards something the session has not
    met yet (coverage()) instead of a draw from the mix.  frames: ("frames", 1 or 2) follows every call."""
    if oracle is None:
        from oracle import oracle as oracle_module
        oracle_module.build()
        oracle = oracle_module
    w = dict(MIX)
    w.update(mix or {})
    anchored = bool(w.pop("relight_anchored", 0))   # relights while the texture origin is not (0, 0)
    names = [k for k in w if w[k] > 0]
    p = np.array([w[k] for k in names], np.float64)
    p /= p.sum()
    rng = np.random.default_rng(seed)
    m = Session(oracle, lg, origin, gi=False)
    X, Y, Z = dims(lg)
    nbx, nbz = X // 8, Z // 8
    hot = [m.key(bx, bz) for bx, bz in ((0, 2), (1, nbz - 2), (nbx - 1, 1), (2, 0), (nbx - 2, nbz - 1), (3, 1))]
    trace, state = [], {"last_edit": None, "puts": 0}
    long_axis = None if max(lg[0], lg[2]) <= 7 else 0 if lg[0] > 7 else 1   # its steps and edits can be local
    n -= len(ending)

    def emit(*op):
        trace.append(op)
        m.apply(op)
        if frames:
            trace.append(("frames", int(rng.integers(1, 3))))

    def pick(seq):
        return seq[int(rng.integers(len(seq)))]

    def home():
        return (origin[0] - m.origin[0], origin[1] - m.origin[1])

    def face(col):
        """(one-axis scroll, axis) that carries column col out through its nearest face."""
        bx, bz = col
        d = min([(8 * (bx + 1), 0), (-8 * (nbx - bx), 0), (0, 8 * (bz + 1)), (0, -8 * (nbz - bz))],
                key=lambda v: abs(v[0]) + abs(v[1]))
        return list(d), 0 if d[0] else 1

    def leave(col, diagonal):
        """The shortest one-axis scroll that carries column col out, or a little further; or diagonal."""
        d, a = face(col)
        d[a] += 8 * int(rng.integers(0, 3)) * (1 if d[a] > 0 else -1)
        if diagonal:
            d[1 - a] = 8 * int(pick([-2, -1, 1, 2]))
        emit("scroll", d[0], d[1])

    def beside(col):
        """The key of a clean column next to col that leaves whenever col leaves through its nearest face."""
        _, a = face(col)
        for s in (1, -1, 2, -2):
            c = (col[0], col[1] + s) if a == 0 else (col[0] + s, col[1])
            if 0 <= c[0] < nbx and 0 <= c[1] < nbz and m.key(*c) not in m.dirty and m.key(*c) not in m.store:
                return m.key(*c)
        return None

    def enter(key):
        """The shortest scroll that brings a key outside the window into it."""
        d = []
        for r, nb in (((key[0] - m.origin[0]) // 8, nbx), ((key[1] - m.origin[1]) // 8, nbz)):
            d.append(8 * (r - (nb - 1)) if r >= nb else 8 * r if r < 0 else 0)
        emit("scroll", d[0], d[1])

    def empty():
        a = int(rng.integers(0, 2))
        d = [0, 0] if rng.uniform() < 0.5 else [8 * int(pick([-2, -1, 1, 2]))] * 2
        d[a] = ((X, Z)[a] + 8 * int(rng.integers(0, 3))) * int(pick([-1, 1]))
        emit("scroll", d[0], d[1])

    def edit(cols, far=None):
        boxes = []
        for _ in range(int(rng.integers(1, 4))):
            u = rng.uniform()
            boxes.append(_small_box(rng, m, pick(cols) if cols and (u < 0.5 or far is False) else
                                    "border" if u < 0.7 else "face" if u < 0.85 else "any"))
        if cols and not any(b[0] >> 3 == c[0] and b[2] >> 3 == c[1] for b in boxes for c in cols):
            boxes[0] = _small_box(rng, m, pick(cols))
        if far or (far is None and rng.uniform() < 0.12):   # the local rebuild is no cheaper than the whole one
            boxes = [_small_box(rng, m, (0, 0)), _small_box(rng, m, (nbx - 1, nbz - 1))]
        state["last_edit"] = tuple(boxes)
        emit("edit", tuple(boxes))

    def put(key):
        state["puts"] += 1
        emit("store_put", key[0], key[1], 100 * (seed % 1000) + state["puts"])

    def outside():
        bx, bz = int(rng.integers(-2, nbx + 2)), int(rng.integers(-2, nbz + 2))
        if 0 <= bx < nbx and 0 <= bz < nbz:
            bx = int(pick([-1, -2, nbx, nbx + 1]))
        return m.key(bx, bz)

    def noop():
        x, y, z = (int(rng.integers(0, v)) for v in (X, Y, Z))
        emit("edit", ((x, y, z, x + 1, y + 1, z + 1, int(m.vox[z, y, x])),))

    def towards(have):
        """The next step towards the first thing the session has not met; False when there is none."""
        back = [c for c in (m.column_of(k) for k in m._restored_once) if c is not None]
        again = [c for c in m.dirty_columns() if m.key(*c) in m._edited_since]
        here = [c for c in (m.column_of(k) for k in hot) if c is not None]
        away = home() != (0, 0)
        if "restore_after_reedit" not in have:
            waiting = any(t == "put" and m.column_of(k) is not None and k not in m.dirty for k, t in m.tag.items())
            if again:
                if "put_overwritten" not in have and m.tag.get(m.key(*again[0])) != "put":
                    put(m.key(*again[0]))
                elif "emptied" not in have:
                    empty()
                else:
                    leave(again[0], "diagonal" not in have)
            elif away and any(t == "captured" for t in m.tag.values()):
                emit("scroll", *home())
            elif back:
                edit(back)
            elif m.dirty_columns():
                col = m.dirty_columns()[0]
                if "put_consumed" not in have and not waiting and beside(col) is not None:
                    put(beside(col))          # a clean neighbour goes out and comes back with it
                else:
                    leave(col, "diagonal" not in have)
            else:
                edit(here)
        elif "put_consumed" not in have:
            puts = [k for k in m.store if m.tag[k] == "put" and m.column_of(k) is None]
            if puts:
                enter(puts[0])
            else:
                put(outside())
        elif "emptied" not in have:
            empty()
        elif "noop_edit" not in have:
            noop()
        elif long_axis is not None and "edit_full" not in have:
            edit(here, far=True)
        elif long_axis is not None and "edit_local" not in have:
            edit(here[:1] or [(1, 1)], far=False)
        elif long_axis is not None and all(full for _, _, full in m.steps):
            emit("scroll", *[8 * int(pick([-1, 1])) if a == long_axis else 0 for a in (0, 1)])
        elif "replaced" not in have and m.dirty_columns():
            emit("flush")
        elif away:
            emit("scroll", *home())
        else:
            return False
        return True

    emit("persist", 1)
    while len(trace) < n:
        have = {e[1] for e in m.log}
        if m.persist_on and rng.uniform() < purpose and towards(have):
            continue
        kind = names[int(rng.choice(len(names), p=p))]
        dirty = m.dirty_columns()
        if kind == "scroll":
            u = rng.uniform()
            if u < 0.08:
                empty()
            elif home() != (0, 0) and u < 0.42:
                emit("scroll", *home())
            elif dirty and u < 0.75:
                leave(pick(dirty), rng.uniform() < 0.25)
            else:
                d = [int(pick([8, 16, 24, 40, 64])) * int(pick([-1, 1])) for _ in range(2)]
                if rng.uniform() < 0.75:      # one axis; the rest are diagonal
                    d[int(rng.integers(0, 2))] = 0
                emit("scroll", d[0], d[1])
        elif kind == "edit":
            edit([c for c in (m.column_of(k) for k in hot) if c is not None])
        elif kind == "noop_edit":
            noop()
        elif kind == "flush":
            emit("flush")
        elif kind == "put_dirty":
            if dirty:
                put(m.key(*pick(dirty)))
        elif kind == "put_clean":
            here = [k for k in hot if m.column_of(k) is not None and k not in m.dirty]
            key = pick(here) if here and rng.uniform() < 0.7 else \
                m.key(int(rng.integers(0, nbx)), int(rng.integers(0, nbz)))
            if key not in m.dirty:
                put(key)
        elif kind == "put_outside":       # a column or two outside a face: the next steps may take it in
            put(outside())
        elif kind == "store_clear":
            emit("store_clear")
        elif kind == "persist_toggle":    # off, one world call without it, and on again
            emit("persist", 0)
            if rng.uniform() < 0.5:
                emit("edit", (_small_box(rng, m, "any"),))
            else:
                emit("scroll", 8 * int(pick([-2, -1, 1, 2])), 0)
            emit("persist", 1)
        elif kind == "texture_origin_set":
            o = m.origin if rng.uniform() < 0.5 else (int(rng.integers(-500, 500)), int(rng.integers(-500, 500)))
            emit("texture_origin_set", o[0], o[1])
        elif kind == "follow_toggle":
            emit("texture_follow_scroll", int(not m.follow))
        elif kind == "relight":
            if state["last_edit"] is not None and (m.tex == (0, 0) or anchored):
                emit("relight", relight_box(lg, state["last_edit"], 1), int(rng.integers(0, 2 ** 32)),
                     int(rng.integers(1, 4)), bool(rng.integers(0, 2)))
        elif kind == "bodies":
            emit("bodies", int(rng.integers(0, 10 ** 6)))
        elif kind == "bad_put":
            emit("bad_put", m.origin[0] + 8 * int(rng.integers(0, nbx)) + int(rng.integers(1, 8)),
                 m.origin[1] + 8 * int(rng.integers(0, nbz)))
        elif kind == "bad_get":
            key = m.key(int(rng.integers(-3, nbx + 3)), int(rng.integers(-3, nbz + 3)))
            if key not in m.store:
                emit("bad_get", *key)
    return trace[:n] + list(ending)
