"""What the Python layer of the eleven frontier choosers hands to the library, pinned without a device and without the library.

Fleet.explore*_stages and Fleet.*_records run here on a Fleet made with Fleet.__new__ whose torch, map, context and stream are stand-ins
that log: every zeros, record_stream and stream context, and every *_goals_device and fleet_set_goals_device with its positional
arguments.  capi.Map.*_goals_device run on a Map made with Map.__new__ over a recording stand-in for capi.lib().  Every expectation is
written out below (argument tuples, the fields of the params records, workspace sizes, allocation order, error texts); none is taken
from the code under test.

The last tests show that the checks bite: a fleet that shares one all-zero view_of between explore() and the others, a fleet whose team
workspace key forgets n, and a map that receives skip and labels in each other's place each fail the check that names them."""
import ctypes

import numpy as np
import pytest

from faster_amd import abi, capi
from faster_amd.fleet import Fleet

N, NV, CELLS, SINGLE = 3, 3, 100, 400     # vehicles, views, cells of a view; cells of set_unknown's one grid
STREAM = 0x5EED
GRID = ((0.0, 0.0, 0.0), 0.5, (5, 5, 4))
Z, WANT = (0.25, 1.75), ("no_path", "all")   # want = 2 | 4


# ---- stand-ins ----
class FakeTensor:
    _next = [0x10000000]

    def __init__(self, shape, dtype, log=None):
        self.shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.dtype, self.log = dtype, log
        self._ptr = FakeTensor._next[0]
        FakeTensor._next[0] += 0x1000

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return int(np.prod(self.shape))

    def record_stream(self, stream):
        self.log.append(("record_stream", self.shape, self.dtype, stream.cuda_stream))

    def cpu(self):
        return self

    def numpy(self):
        return np.zeros(self.shape, dtype=self.dtype)


class FakeTorch:
    uint8, int32, float64 = "uint8", "int32", "float64"

    def __init__(self, log):
        self.log, self.cuda = log, self

    def zeros(self, shape, dtype, device):
        self.log.append(("zeros", shape, dtype, device))
        return FakeTensor(shape, dtype, self.log)

    def stream(self, stream):   # torch.cuda.stream
        log = self.log

        class Ctx:
            def __enter__(self):
                log.append(("enter", stream.cuda_stream))

            def __exit__(self, *exc):
                log.append(("exit",))

        return Ctx()


class FakeStream:
    cuda_stream = STREAM


class Recorder:
    """Every method called on it is logged as (kind, name, positional arguments)."""

    def __init__(self, log, kind):
        self.log, self.kind = log, kind

    def __getattr__(self, name):
        if not name.endswith("_device"):
            raise AttributeError(name)
        return lambda *args: self.log.append((self.kind, name, args))


def grid_at(p):
    return np.frombuffer(ctypes.string_at(p.value, abi.voxel_grid_dtype.itemsize), dtype=abi.voxel_grid_dtype)[0]


class FleetLib:
    """capi.lib() as Fleet uses it: the four workspace sizes, each a different function of every argument it is given."""

    @staticmethod
    def fh_spread_work_bytes(n):
        return 1000 + n

    @staticmethod
    def fh_bid_work_bytes(n):
        return 2000 + n

    @staticmethod
    def _lattice(base, g, block, n_views, n=0):
        return base + 100 * int(grid_at(g)["dims"].sum()) + 10 * block + n_views + 1000 * n if 1 <= block <= 16 else 0

    def fh_far_work_bytes(self, g, block, n_views):
        return self._lattice(10000, g, block, n_views)

    def fh_prospect_work_bytes(self, g, block, n_views):
        return self._lattice(20000, g, block, n_views)

    def fh_apart_work_bytes(self, g, block, n_views, n):
        return self._lattice(30000, g, block, n_views, n)

    def fh_stake_work_bytes(self, g, block, n_views, n):
        return self._lattice(40000, g, block, n_views, n)


NAMES = ("explore", "reach", "spread", "gain", "team", "sight", "bid", "far", "far_spread", "far_gain", "far_team")
WITH_WORK = ("spread", "team", "bid", "far", "far_spread", "far_gain", "far_team")
WITH_KEY = ("far", "far_spread", "far_gain", "far_team")


def make_fleet(monkeypatch, views=True, view_of=True, cls=Fleet):
    """A fleet after set_map, enable_heading and set_unknown_views (views=False: set_unknown), before any chooser has run."""
    monkeypatch.setattr(capi, "lib", lambda: FleetLib())
    log = []
    f = cls.__new__(cls)
    f.log, f.torch, f.dev, f.stream = log, FakeTorch(log), "dev", FakeStream()
    f.map, f.ctx = Recorder(log, "map"), Recorder(log, "ctx")
    f._follow_current = lambda: log.append(("follow",))
    f.sync = lambda: log.append(("sync",))
    f.n, f.params, f.z_ground = N, abi.default_fleet_params(), 0.125
    f.params["goal_radius"] = 0.625
    f.cloud, f.map_args, f.grid = object(), ((10, 10, 4), 0.2, (0.0, 0.0, 1.0), 2.0, 0.0), GRID
    f.d_headings, f.d_vehicles, f.d_link_labels = object(), FakeTensor(N * 8, "uint8"), None
    if views:
        f.view_flags, f.flags, f.n_views = FakeTensor((NV, CELLS), "uint8"), None, NV
        f.view_of = FakeTensor(N, "int32") if view_of else None
    else:
        f.view_flags, f.flags, f.n_views, f.view_of = None, FakeTensor(SINGLE, "uint8"), 0, None
    for name in NAMES:
        for what in ("goals", "mask", "records"):
            setattr(f, "d_%s_%s" % (name, what), None)
    for name in WITH_WORK:
        setattr(f, "d_%s_work" % name, None)
    for name in WITH_KEY:
        setattr(f, "_%s_work_key" % name, None)
    f.d_explore_view_of = f.d_reach_view_of = None
    return f


def symbols(f, args):
    """The arguments of a logged call with every pointer replaced by the name of the fleet's attribute that holds that tensor, the
    params record by "par" and the fleet's grid and params by "grid" and "params"."""
    names = {v.data_ptr(): k for k, v in vars(f).items() if isinstance(v, FakeTensor)}
    out = []
    for a in args:
        if a is f.grid:
            out.append("grid")
        elif a is f.params:
            out.append("params")
        elif isinstance(a, np.ndarray):
            out.append("par")
        else:
            out.append(names.get(a, a) if isinstance(a, int) else a)
    return tuple(out)


def launch(f, stages):
    """Runs the stages; -> (the names, the goals call as (method, symbolic arguments, par), the set_goals call likewise)."""
    del f.log[:]
    for _, run in stages:
        run()
    assert [e[0] for e in f.log] == ["map", "ctx"], f.log
    (_, method, args), (_, setter, sargs) = f.log
    par = [a for a in args if isinstance(a, np.ndarray)]
    assert len(par) == 1 and args[0] is par[0]
    return [n for n, _ in stages], (method, symbols(f, args), par[0]), (setter, symbols(f, sargs))


def record(dtype, fields):
    """One record of `dtype` with the named fields set and every reserved field zero; every other field must be named."""
    assert set(fields) == {n for n in dtype.names if not n.startswith("reserved")}, sorted(fields)
    p = np.zeros((), dtype=dtype)
    for k, v in fields.items():
        p[k] = v
    return p


def alloc_log(*groups):
    """The log of lazy allocations: per group _follow_current, the fleet's stream entered, the zeros, the stream left, then
    record_stream on each new tensor in the same order."""
    out = []
    for group in groups:
        out += [("follow",), ("enter", STREAM)] + [("zeros", shape, dtype, "dev") for shape, dtype in group] + [("exit",)]
        out += [("record_stream", (shape,) if isinstance(shape, int) else shape, dtype, STREAM) for shape, dtype in group]
    return out


# ---- the eleven choosers: how they are called, and what has to come out ----
def outputs(record_bytes):
    return [((N, 3), "float64"), (N, "int32"), (N * record_bytes, "uint8")]


def args_plain(name, view_of, stream=True):
    return ("par", "grid", "view_flags", CELLS, view_of, NV, "d_vehicles", N, "d_%s_goals" % name, "d_%s_mask" % name,
            "d_%s_records" % name) + ((STREAM,) if stream else ())


def args_team(name, view_of, work_bytes, labels=None):
    return ("par", "grid", "view_flags", CELLS, view_of, NV, labels, "d_vehicles", N, "d_%s_work" % name, work_bytes, "d_%s_goals" % name,
            "d_%s_mask" % name, "d_%s_records" % name, STREAM)


def args_far(name, view_of, work_bytes, skip=None):
    return ("par", "grid", "view_flags", CELLS, view_of, NV, skip, "d_vehicles", N, "d_%s_work" % name, work_bytes, "d_%s_goals" % name,
            "d_%s_mask" % name, "d_%s_records" % name, STREAM)


def args_far_team(name, view_of, work_bytes, skip=None, labels=None):
    return ("par", "grid", "view_flags", CELLS, view_of, NV, skip, labels, "d_vehicles", N, "d_%s_work" % name, work_bytes,
            "d_%s_goals" % name, "d_%s_mask" % name, "d_%s_records" % name, STREAM)


NEAR = dict(r_max=2.5, r_avoid=0.75, z_lo=0.25, z_hi=1.75, want=6)             # what every explicit call below asks for
NEAR0 = dict(r_max=2.5, r_avoid=0.625, z_lo=0.125, z_hi=2.0, want=1)           # and what the defaults give: goal_radius, z_ground, z_max
FAR = dict(r_avoid=0.75, z_lo=0.25, z_hi=1.75, want=6, max_hops=7, block=8)
FAR0 = dict(r_avoid=0.625, z_lo=0.125, z_hi=2.0, want=1, max_hops=0, block=8)

# name: (run, stages, records, record dtype, its bytes, params dtype, Map method, stage, workspace bytes, shape of the arguments,
#        explicit positional arguments, the fields they give, the fewest arguments, the fields they give)
CASES = {
    "explore": ("explore", "explore_stages", "explore_records", abi.frontier_record_dtype, 32, abi.frontier_params_dtype,
                "frontier_goals_device", "frontier_goals", None, "plain",
                (2.5, 0.75, Z, WANT), NEAR, (2.5,), NEAR0),
    "reach": ("explore_reachable", "explore_reachable_stages", "reach_records", abi.reach_record_dtype, 48, abi.reach_params_dtype,
              "reach_goals_device", "reach_goals", None, "plain",
              (2.5, 0.75, Z, WANT, 7), dict(NEAR, max_hops=7), (2.5,), dict(NEAR0, max_hops=0)),
    "spread": ("explore_spread", "explore_spread_stages", "spread_records", abi.spread_record_dtype, 64, abi.spread_params_dtype,
               "spread_goals_device", "spread_goals", 1003, "team",
               (2.5, 1.5, 0.75, Z, WANT, 7, 5, "view"), dict(NEAR, max_hops=7, r_spread=1.5, passes=5),
               (2.5, 1.5), dict(NEAR0, max_hops=0, r_spread=1.5, passes=8)),
    "gain": ("explore_gain", "explore_gain_stages", "gain_records", abi.gain_record_dtype, 64, abi.gain_params_dtype,
             "gain_goals_device", "gain_goals", None, "plain",
             (2.5, 4, 3, 2, 0.75, Z, WANT, 7), dict(NEAR, max_hops=7, gain_radius=4, hop_cost=3, min_gain=2),
             (2.5, 4), dict(NEAR0, max_hops=0, gain_radius=4, hop_cost=1, min_gain=0)),
    "sight": ("explore_sight", "explore_sight_stages", "sight_records", abi.sight_record_dtype, 64, abi.sight_params_dtype,
              "sight_goals_device", "sight_goals", None, "plain",
              (2.5, 4, 3, 2, 0.75, Z, WANT, 7), dict(NEAR, max_hops=7, gain_radius=4, hop_cost=3, min_gain=2),
              (2.5, 4), dict(NEAR0, max_hops=0, gain_radius=4, hop_cost=1, min_gain=0)),
    "team": ("explore_team", "explore_team_stages", "team_records", abi.team_record_dtype, 96, abi.team_params_dtype,
             "team_goals_device", "team_goals", 1003, "team",
             (2.5, 1.5, 4, 6, 3, 2, 0.75, Z, WANT, 7, 5, "view"),
             dict(NEAR, max_hops=7, r_spread=1.5, passes=5, gain_radius=4, hop_cost=3, min_gain=2, claim_radius=6),
             (2.5, 1.5, 4), dict(NEAR0, max_hops=0, r_spread=1.5, passes=8, gain_radius=4, hop_cost=1, min_gain=0, claim_radius=4)),
    "bid": ("explore_bid", "explore_bid_stages", "bid_records", abi.bid_record_dtype, 96, abi.bid_params_dtype,
            "bid_goals_device", "bid_goals", 2003, "team",
            (2.5, 1.5, 4, 6, 3, 2, 0.75, Z, WANT, 7, 5, "view"),
            dict(NEAR, max_hops=7, r_spread=1.5, passes=5, gain_radius=4, hop_cost=3, min_gain=2, claim_radius=6),
            (2.5, 1.5, 4), dict(NEAR0, max_hops=0, r_spread=1.5, passes=8, gain_radius=4, hop_cost=1, min_gain=0, claim_radius=4)),
    "far": ("explore_far", "explore_far_stages", "far_records", abi.far_record_dtype, 64, abi.far_params_dtype,
            "far_goals_device", "far_goals", 11483, "far",
            (8, 0.75, Z, WANT, 7, None), FAR, (), FAR0),
    "far_gain": ("explore_far_gain", "explore_far_gain_stages", "far_gain_records", abi.far_gain_record_dtype, 80, abi.far_gain_params_dtype,
                 "far_gain_goals_device", "far_gain_goals", 21483, "far",
                 (8, 3, 50, 2, 0.75, Z, WANT, 7, None), dict(FAR, gain_blocks=3, hop_cost=50, min_gain=2),
                 (), dict(FAR0, gain_blocks=2, hop_cost=64, min_gain=0)),
    "far_spread": ("explore_far_spread", "explore_far_spread_stages", "far_spread_records", abi.far_spread_record_dtype, 96,
                   abi.far_spread_params_dtype, "far_spread_goals_device", "far_spread_goals", 34483, "far_team",
                   (8, 1.5, 0.75, Z, WANT, 7, 5, "view", None), dict(FAR, r_spread=1.5, passes=5),
                   (), dict(FAR0, r_spread=2.0, passes=8)),
    "far_team": ("explore_far_team", "explore_far_team_stages", "far_team_records", abi.far_team_record_dtype, 128, abi.far_team_params_dtype,
                 "far_team_goals_device", "far_team_goals", 44483, "far_team",
                 (8, 1.5, 3, 50, 2, 4, 0.75, Z, WANT, 7, 5, "view", None),
                 dict(FAR, gain_blocks=3, hop_cost=50, min_gain=2, r_spread=1.5, passes=5, claim_blocks=4),
                 (), dict(FAR0, gain_blocks=2, hop_cost=64, min_gain=0, r_spread=2.0, passes=8, claim_blocks=2)),
}
assert tuple(sorted(CASES)) == tuple(sorted(NAMES))


def expected_args(name, view_of):
    shape, work_bytes = CASES[name][9], CASES[name][8]
    if shape == "plain":
        return args_plain(name, view_of, stream=name != "explore")
    return {"team": args_team, "far": args_far, "far_team": args_far_team}[shape](name, view_of, work_bytes)


def expected_allocs(name, views=NV):
    """Outputs and, for a team, its workspace in one block; the far choosers' workspace in a block of its own behind them (its size
    counts the views)."""
    shape, work_bytes, out = CASES[name][9], CASES[name][8], outputs(CASES[name][4])
    if shape == "plain":
        return alloc_log(out)
    if shape == "team":
        return alloc_log(out + [(work_bytes, "uint8")])
    return alloc_log(out, [(work_bytes - NV + views, "uint8")])


@pytest.mark.parametrize("name", NAMES)
def test_stage_names_arguments_params_and_allocation(name, monkeypatch):
    run, stages_of, _, _, _, pdt, method, stage, _, _, explicit, fields, fewest, fields0 = CASES[name]
    # the fewest arguments, no view_of: every default of the Python layer
    f = make_fleet(monkeypatch, view_of=False)
    stages = getattr(f, stages_of)(*fewest)
    assert f.log == expected_allocs(name)   # (allocated when the stages are built: order, shapes, stream discipline)
    names, (m, args, par), setter = launch(f, stages)
    assert names == [stage, "set_goals"]
    assert m == method and args == expected_args(name, None)
    assert par.dtype == pdt and par.tobytes() == record(pdt, fields0).tobytes(), par
    assert setter == ("fleet_set_goals_device", ("params", "d_vehicles", "d_%s_goals" % name, "d_%s_mask" % name, N))
    # every argument given, a view_of: the same buffers, nothing allocated again
    f.view_of = FakeTensor(N, "int32")
    held = {k: v for k, v in vars(f).items() if isinstance(v, FakeTensor)}
    del f.log[:]
    stages = getattr(f, stages_of)(*explicit)
    assert f.log == []
    assert {k: v for k, v in vars(f).items() if isinstance(v, FakeTensor)} == held
    names, (m, args, par), setter = launch(f, stages)
    assert names == [stage, "set_goals"]
    assert m == method and args == expected_args(name, "view_of")
    assert par.dtype == pdt and par.tobytes() == record(pdt, fields).tobytes(), par
    assert setter == ("fleet_set_goals_device", ("params", "d_vehicles", "d_%s_goals" % name, "d_%s_mask" % name, N))
    # explore_X(): the stages, then _follow_current, then the two launches
    del f.log[:]
    getattr(f, run)(*explicit)
    assert [e[:2] for e in f.log] == [("follow",), ("map", method), ("ctx", "fleet_set_goals_device")]
    assert symbols(f, f.log[1][2]) == expected_args(name, "view_of")


@pytest.mark.parametrize("name", NAMES)
def test_records_before_and_after(name, monkeypatch):
    run, stages_of, records, rdt, rbytes, *_ = CASES[name]
    fewest = CASES[name][12]
    f = make_fleet(monkeypatch)
    with pytest.raises(capi.FasterHipError) as e:
        getattr(f, records)()
    assert str(e.value) == "Fleet.%s: %s first" % (records, run)
    getattr(f, stages_of)(*fewest)
    del f.log[:]
    rec, goals, mask = getattr(f, records)()
    assert f.log == [("sync",)]
    assert rec.dtype == rdt and rec.shape == (N,) and rdt.itemsize == rbytes
    assert (goals.dtype, goals.shape, mask.dtype, mask.shape) == (np.float64, (N, 3), np.int32, (N,))


@pytest.mark.parametrize("name,with_n", [("far", False), ("far_gain", False), ("far_spread", True), ("far_team", True)])
def test_far_workspace_follows_its_key_and_nothing_else_does(name, with_n, monkeypatch):
    stages_of, method, base = CASES[name][1], CASES[name][6], CASES[name][8] - 1483 - (3000 if with_n else 0)
    f = make_fleet(monkeypatch)
    getattr(f, stages_of)()
    outs = [getattr(f, "d_%s_%s" % (name, w)) for w in ("goals", "mask", "records")]

    def again(what, work_bytes, **kw):
        """The stages once more: work_bytes None: nothing is allocated; else the workspace alone, with that many bytes."""
        work = getattr(f, "d_%s_work" % name)
        del f.log[:]
        stages = getattr(f, stages_of)(**kw)
        assert f.log == ([] if work_bytes is None else alloc_log([(work_bytes, "uint8")])), (what, f.log)
        assert (getattr(f, "d_%s_work" % name) is work) == (work_bytes is None)
        assert [getattr(f, "d_%s_%s" % (name, w)) for w in ("goals", "mask", "records")] == outs
        _, (_, args, _), _ = launch(f, stages)
        assert args[-6:-4] == ("d_%s_work" % name, getattr(f, "d_%s_work" % name).numel())   # (the new one, and its size)

    n_part = 3000 if with_n else 0
    again("nothing changed", None)
    again("block changed", base + 1400 + 40 + 3 + n_part, block=4)
    again("nothing changed", None, block=4)
    f.grid = (GRID[0], GRID[1], (6, 5, 4))
    again("lattice changed", base + 1500 + 40 + 3 + n_part, block=4)
    f.view_flags, f.n_views = FakeTensor((5, CELLS), "uint8"), 5
    again("n_views changed", base + 1500 + 40 + 5 + n_part, block=4)
    f.n = 4
    again("n changed", base + 1500 + 40 + 5 + 4000 if with_n else None, block=4)   # (only where the workspace holds a row per vehicle)
    again("nothing changed", None, block=4)
    assert f.log[0][1] == method


def zero_view_of_check(f):
    """set_unknown's one grid: explore() makes its all-zero view_of once, the other ten share another, made once."""
    for name in NAMES:
        stages_of, fewest = CASES[name][1], CASES[name][12]
        attr = "d_explore_view_of" if name == "explore" else "d_reach_view_of"
        for i in range(2):
            had = getattr(f, attr)
            assert (had is None) == (i == 0 and name in ("explore", "reach")), (name, i)
            del f.log[:]
            stages = getattr(f, stages_of)(*fewest)
            assert f.log == (alloc_log([(N, "int32")]) if had is None else []) + (expected_allocs(name, views=1) if i == 0 else []), (name, i)
            assert had is None or getattr(f, attr) is had, name
            _, (_, args, _), _ = launch(f, stages)
            assert args[2:6] == ("flags", SINGLE, attr, 1), (name, args)
    assert f.d_explore_view_of is not f.d_reach_view_of


def test_single_grid_makes_each_zero_view_of_once(monkeypatch):
    zero_view_of_check(make_fleet(monkeypatch, views=False))


AFTER = {"explore": "d_explore_mask", "reachable": "d_reach_mask", "spread": "d_spread_mask", "gain": "d_gain_mask", "sight": "d_sight_mask",
         "team": "d_team_mask", "bid": "d_bid_mask"}


@pytest.mark.parametrize("name", WITH_KEY)
def test_after_reaches_the_mask_of_that_chooser(name, monkeypatch):
    stages_of = CASES[name][1]
    f = make_fleet(monkeypatch)
    for after, attr in AFTER.items():
        with pytest.raises(capi.FasterHipError) as e:
            getattr(f, stages_of)(after=after)
        assert str(e.value) == "Fleet.%s: after=%r, but that chooser has not run" % (CASES[name][0], after)
    for attr in AFTER.values():
        setattr(f, attr, FakeTensor(N, "int32"))
    for after, attr in AFTER.items():
        _, (_, args, _), _ = launch(f, getattr(f, stages_of)(after=after))
        assert args == expected_args(name, "view_of")[:6] + (attr,) + expected_args(name, "view_of")[7:], (after, args)
    with pytest.raises(capi.FasterHipError) as e:
        getattr(f, stages_of)(after="nearest")
    assert str(e.value) == ("Fleet.%s: after is None or one of bid, explore, gain, reachable, sight, spread, team, got 'nearest'" % CASES[name][0])


def labels_check(name, f_views, f_single):
    """groups="link" hands the labels of the last link() over only where there are views and a label per view."""
    stages_of, fewest = CASES[name][1], CASES[name][12]
    at = 7 if CASES[name][9] == "far_team" else 6

    def labels(f, **kw):
        _, (_, args, _), _ = launch(f, getattr(f, stages_of)(*fewest, **kw))
        return args[at]

    assert labels(f_views) is None                       # no link() yet
    f_views.d_link_labels = FakeTensor(NV, "int32")
    assert labels(f_views) == "d_link_labels"
    assert labels(f_views, groups="link") == "d_link_labels"
    assert labels(f_views, groups="view") is None
    f_views.d_link_labels = FakeTensor(NV + 1, "int32")   # a link() of other views
    assert labels(f_views) is None
    f_single.d_link_labels = FakeTensor(1, "int32")       # set_unknown's one grid: nothing to label, whatever the count
    assert labels(f_single) is None
    with pytest.raises(capi.FasterHipError) as e:
        getattr(f_views, stages_of)(*fewest, groups="team")
    assert str(e.value) == "Fleet.%s: groups is \"link\" or \"view\", got 'team'" % CASES[name][0]


@pytest.mark.parametrize("name", ("spread", "team", "bid", "far_spread", "far_team"))
def test_groups_link_takes_the_labels_only_when_they_fit_the_views(name, monkeypatch):
    labels_check(name, make_fleet(monkeypatch), make_fleet(monkeypatch, views=False))


def test_groups_is_checked_before_set_map_and_block_between_after_and_gain_blocks(monkeypatch):
    f = make_fleet(monkeypatch)
    f.cloud = None
    for name in ("spread", "team", "bid", "far_spread", "far_team"):
        run, fewest = CASES[name][0], CASES[name][12]
        with pytest.raises(capi.FasterHipError, match="groups is"):
            getattr(f, run)(*fewest, groups="team")
        with pytest.raises(capi.FasterHipError) as e:
            getattr(f, run)(*fewest)
        assert str(e.value) == "Fleet.%s: set_map first" % run
    f = make_fleet(monkeypatch)
    with pytest.raises(capi.FasterHipError, match="after is None"):
        f.explore_far_team(17, gain_blocks=9, after="nearest")
    with pytest.raises(capi.FasterHipError) as e:
        f.explore_far_team(17, gain_blocks=9)
    assert str(e.value) == ("Fleet.explore_far_team: block must be 1 .. 16 and the blocks of the lattice must fit 512 words of 64 (got block 17 "
                            "on a lattice of (5, 5, 4))")
    with pytest.raises(capi.FasterHipError, match="gain_blocks must be 0 .. 5"):
        f.explore_far_team(8, gain_blocks=9)
    assert f.log == []   # (nothing was allocated on the way to an error)


# ---- capi.Map: the ten wrappers over the library's entry points ----
MAP_DIMS, MAP_ORIGIN, MAP_RES, MAP_BITS, HANDLE = (7, 6, 5), (-1.0, -2.0, 0.5), 0.25, 0xB175, 0x4A9


class MapLib:
    """capi.lib() as Map uses it: fh_map_dims and fh_map_occupancy_bits_device answer with the constants above, every goals entry point
    logs (symbol, arguments), with the records behind the three pointers read while the call runs, and returns `rc`."""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def fh_map_dims(self, h, d, o):
        assert h == HANDLE
        ctypes.memmove(d, np.array(MAP_DIMS, dtype=np.int32).ctypes.data, 12)
        ctypes.memmove(o, np.array(MAP_ORIGIN, dtype=np.float64).ctypes.data, 24)
        return 0

    def fh_map_occupancy_bits_device(self, h, bits, res):
        assert h == HANDLE
        bits._obj.value, res._obj.value = MAP_BITS, MAP_RES
        return 0

    def fh_map_last_error(self, h):
        return b""

    def __getattr__(self, symbol):
        if not symbol.endswith("_goals_device"):
            raise AttributeError(symbol)

        def call(stream, par, map_grid, bits, grid, *rest):
            mg, g = grid_at(map_grid), (None if grid is None else grid_at(grid))
            self.calls.append((symbol, stream, ctypes.string_at(par.value, self.par_bytes), (tuple(mg["origin"]), float(mg["res"]), tuple(mg["dims"])),
                               bits.value, None if g is None else (tuple(g["origin"]), float(g["res"]), tuple(g["dims"])), rest))
            return self.rc

        return call


# wrapper: (symbol, the params of abi.default_*_params, which of d_skip and d_group it takes, whether it takes d_work and work_bytes)
WRAPPERS = {
    "reach_goals_device": ("fh_reach_goals_device", abi.default_reach_params(2.5), "", False),
    "gain_goals_device": ("fh_gain_goals_device", abi.default_gain_params(2.5, 4), "", False),
    "sight_goals_device": ("fh_sight_goals_device", abi.default_sight_params(2.5, 4), "", False),
    "spread_goals_device": ("fh_spread_goals_device", abi.default_spread_params(2.5, 1.5), "g", True),
    "team_goals_device": ("fh_team_goals_device", abi.default_team_params(2.5, 1.5, 4), "g", True),
    "bid_goals_device": ("fh_bid_goals_device", abi.default_bid_params(2.5, 1.5, 4), "g", True),
    "far_goals_device": ("fh_far_goals_device", abi.default_far_params(8), "s", True),
    "far_gain_goals_device": ("fh_prospect_goals_device", abi.default_far_gain_params(8, 2), "s", True),
    "far_spread_goals_device": ("fh_apart_goals_device", abi.default_far_spread_params(8, 2.0), "sg", True),
    "far_team_goals_device": ("fh_stake_goals_device", abi.default_far_team_params(8, 2.0, 2), "sg", True),
}


class Intish:
    """Converts with int() and equals no int: a wrapper that forgets the conversion passes it on as it is."""

    def __init__(self, v):
        self.v = v

    def __int__(self):
        return self.v


def map_call(wrapper, par, grid, m=None):
    """The wrapper called with a distinct value in every position; -> the positional arguments."""
    _, _, middle, work = WRAPPERS[wrapper]
    args = [par, grid, 0xF1A65, Intish(CELLS), 0x71E0F, Intish(NV)]
    args += [0x5C19] if "s" in middle else []
    args += [0x6209] if "g" in middle else []
    args += [0x7E41C, Intish(N)]
    args += [0x3029, Intish(4321)] if work else []
    args += [0x60A15, 0x3A5C, 0x9EC5, STREAM]
    m = m or capi.Map.__new__(capi.Map)
    m._h = HANDLE
    try:
        return getattr(m, wrapper)(*args)
    finally:
        m._h = None   # (nothing for Map.__del__ to destroy)


def expected_rest(wrapper):
    _, _, middle, work = WRAPPERS[wrapper]
    return ((0xF1A65, CELLS, 0x71E0F, NV) + ((0x5C19,) if "s" in middle else ()) + ((0x6209,) if "g" in middle else ()) + (0x7E41C, N)
            + ((0x3029, 4321) if work else ()) + (0x60A15, 0x3A5C, 0x9EC5))


def map_wrapper_check(wrapper, monkeypatch, m=None):
    symbol, par, _, _ = WRAPPERS[wrapper]
    L = MapLib()
    L.par_bytes = par.dtype.itemsize
    monkeypatch.setattr(capi, "lib", lambda: L)
    map_call(wrapper, par, GRID, m)
    assert len(L.calls) == 1
    got_symbol, stream, par_bytes, map_grid, bits, grid, rest = L.calls[0]
    assert got_symbol == symbol and stream == STREAM and par_bytes == par.tobytes()
    assert map_grid == (MAP_ORIGIN, MAP_RES, MAP_DIMS) and bits == MAP_BITS and grid == GRID
    assert rest == expected_rest(wrapper) and all(type(a) is int for a in rest), rest
    map_call(wrapper, par, None, m)   # (no grid of the views: a null pointer)
    assert L.calls[1][5] is None and L.calls[1][6] == expected_rest(wrapper)


@pytest.mark.parametrize("wrapper", sorted(WRAPPERS))
def test_map_wrapper_symbol_positions_and_conversions(wrapper, monkeypatch):
    map_wrapper_check(wrapper, monkeypatch)


@pytest.mark.parametrize("wrapper", sorted(WRAPPERS))
def test_map_wrapper_errors(wrapper, monkeypatch):
    symbol, par, _, _ = WRAPPERS[wrapper]
    L = MapLib(rc=-7)
    L.par_bytes = par.dtype.itemsize
    monkeypatch.setattr(capi, "lib", lambda: L)
    with pytest.raises(capi.FasterHipError) as e:
        map_call(wrapper, par, GRID)
    assert str(e.value) == "%s: rc=-7" % symbol
    name = wrapper[:-len("_goals_device")]
    del L.calls[:]
    for bad, said in ((abi.default_frontier_params(2.5), "got dtype %s, 1 elements" % abi.frontier_params_dtype),
                      (np.stack([par, par]), "got dtype %s, 2 elements" % par.dtype)):
        with pytest.raises(capi.FasterHipError) as e:
            map_call(wrapper, bad, GRID)
        assert str(e.value) == "%s: par must be one abi.%s_params_dtype record (abi.default_%s_params), %s" % (wrapper, name, name, said)
    assert L.calls == []


# ---- the checks above are sharp: three one-line mutants, each caught by the check that names it ----
class SharedZeroViewOf(Fleet):
    """explore() uses d_reach_view_of."""
    d_explore_view_of = property(lambda self: self.d_reach_view_of, lambda self, v: setattr(self, "d_reach_view_of", v))


class TeamKeyWithoutN(Fleet):
    """The key of explore_far_team()'s workspace leaves out n: a key that differs in n alone compares equal."""
    _far_team_work_key = property(lambda self: self._key and self._key[:3] + (self.n,), lambda self, v: setattr(self, "_key", v))


class SkipAndLabelsSwapped(capi.Map):
    """far_team_goals_device hands d_skip and d_group over in each other's place."""

    def far_team_goals_device(self, par, grid, d_flags, view_stride, d_view_of, n_views, d_skip, d_group, *rest):
        return capi.Map.far_team_goals_device(self, par, grid, d_flags, view_stride, d_view_of, n_views, d_group, d_skip, *rest)


def test_mutant_explore_on_d_reach_view_of_is_caught(monkeypatch):
    with pytest.raises(AssertionError, match="'explore'.*'d_reach_view_of'"):
        zero_view_of_check(make_fleet(monkeypatch, views=False, cls=SharedZeroViewOf))


def test_mutant_workspace_key_without_n_is_caught(monkeypatch):
    real = make_fleet

    def mutant(monkeypatch, **kw):
        return real(monkeypatch, cls=TeamKeyWithoutN, **kw)

    monkeypatch.setitem(globals(), "make_fleet", mutant)
    with pytest.raises(AssertionError, match="n changed"):
        test_far_workspace_follows_its_key_and_nothing_else_does("far_team", True, monkeypatch)


def test_mutant_skip_and_labels_swapped_is_caught(monkeypatch):
    m = SkipAndLabelsSwapped.__new__(SkipAndLabelsSwapped)
    map_wrapper_check("far_team_goals_device", monkeypatch)
    with pytest.raises(AssertionError, match="%d, %d" % (0x6209, 0x5C19)):   # (d_group where d_skip belongs)
        map_wrapper_check("far_team_goals_device", monkeypatch, m)
