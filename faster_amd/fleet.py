"""A fleet of vehicles replanning in steady state on the device (fh_fleet_*, include/fasterhip.h).

Faster::replan (faster/src/faster.cpp:296-595) runs once per period and carries its plan, its status and its two factor windows from one
call to the next.  `Fleet` keeps that state for N vehicles in device memory and runs one period of all of them as a fixed chain of batch
launches on one stream, with no host round trip inside:

    begin -> path search (sphere per vehicle) -> corridors -> corridor problems -> whole solve -> safe corridor -> safe solve -> commit

All vehicles share one map of occupied space per cycle (set_map).  Unknown space is either one grid for the whole fleet (set_unknown) or a
view per vehicle or team (set_unknown_views) that the vehicles grow on the device by looking around (sense): a closed-loop period is then

    sense -> replan -> next_goals

with no host data in it.  set_point_views() gives every view its own knowledge of OCCUPIED space as well — a mask over the points of the
shared cloud that observe() grows from what the view has seen — and the loop becomes

    sense -> observe -> replan -> next_goals

in which a vehicle searches its path and cuts both corridors around the points its view knows, and no others.  enable_traffic() makes
the vehicles avoid each other with the same mechanism: traffic() writes the committed plans of the other vehicles as points at the tail
of the cloud and sets, in the mask row of vehicle i, the bits of those it has to keep clear of (include/fasterhip_traffic.h: the samples
near where vehicle i stands; with timed=True include/fasterhip_traffic_timed.h: the samples its own plan comes near at the same instant):

    sense -> observe -> traffic -> replan -> next_goals

enable_obstacles() does the same for things that move and are no fleet member (include/fasterhip_obstacles.h): obstacles() writes the
predicted positions of balls that fly a straight line behind the traffic's points and shows vehicle i the samples its own plan comes
near at the same instant; obstacle_audit() measures what the fleet flies against where they are at the same instant:

    sense -> observe -> traffic -> obstacles -> replan -> next_goals

enable_tracking() takes the host out of that loop (include/fasterhip_track.h): track() decides on the device which obstacles some vehicle
sees now (in range, no wall of the map between), keeps a ring of sightings per obstacle, fits a constant velocity to it and writes the
records that obstacles() reads:

    sense -> observe -> traffic -> track -> obstacles -> replan -> next_goals

enable_check() lets the fleet refuse: every commit is compared, instant by instant, with the other vehicles' plans and taken back when it
conflicts (include/fasterhip_check.h); the chain ends ... -> safe solve -> backup -> commit -> check -> revert.

enable_rounds() splits a replan into priority rounds (include/fasterhip_rounds.h): vehicles whose plans come near each other replan in
different rounds, and a later round sees, through traffic and check, what the earlier ones committed moments ago:

    begin -> round_classes -> for every round: gate -> [traffic] -> path search -> ... -> commit [-> check -> revert] -> gate_restore

enable_listed_views() makes map_views cheap where few vehicles replan (include/fasterhip_view_subset.h): a view_list stage lists, on the
device, the views of the vehicles that are switched on, and map_views rebuilds the grids and jump tables of those views only.

link() lets the vehicles in radio range of each other pool what their views know (include/fasterhip_link.h): the views of every connected
group become equal, unknown voxels and occupied points alike, and the group plans as a team does until it parts; link(range, los=True) is
the same where walls block a link (include/fasterhip_link_los.h: a pair needs a line of sight through the fleet's map):

    sense -> observe -> link -> replan -> next_goals

explore() closes the loop (include/fasterhip_frontier.h): a vehicle that has arrived takes the nearest voxel of its view that is known,
free and next to unknown space as its new goal, on the device; coverage() counts what every view knows, so a loop can tell when it is done:

    sense -> observe -> [link] -> explore -> replan -> next_goals

explore_reachable() stands in explore()'s place (include/fasterhip_reach.h): of those voxels the one that a flood of the space the view
knows to be free reaches in the fewest steps, never one behind a wall or in a sealed pocket.  explore_spread() is that chooser for a team
(include/fasterhip_spread.h): a voxel nearer than r_spread to the goal a peer holds or has just been given is left to that peer.
explore_gain() is explore_reachable() with a sense of what a goal is worth (include/fasterhip_gain.h): the unknown voxels near a
candidate are weighed against the steps to it.  explore_sight() is explore_gain() with the sensor's occlusion
(include/fasterhip_sight.h): an unknown voxel counts only if no voxel known to be occupied lies on the line from the candidate to it.
explore_bid() is explore_team() with rounds ordered by bids (include/fasterhip_bid.h): of two teammates before one goal the one with the
better offer gets it, whatever its index, and the other searches again under the winner's claim.

explore_far() is the fallback behind all of them (include/fasterhip_far.h).  Those choosers search the box of the vehicle's r_max sphere;
a vehicle whose frontiers all lie beyond it gets no goal and stays where it is.  explore_far(after=<that chooser>) floods the WHOLE view
at the resolution of blocks of voxels and gives every vehicle the chooser left without a goal the nearest frontier a chain of linked
blocks reaches, however far away it is:

    sense -> observe -> [link] -> explore_reachable -> explore_far(after="reachable") -> replan -> next_goals

explore_far_gain() is explore_far() with a gain (include/fasterhip_prospect.h): a target block is weighed by the unknown voxels of the
blocks around it, and the best  gain - hop_cost * hops  of all levels of the flood is taken, not the first target block the flood meets.

explore_far_spread() is explore_far() for a team (include/fasterhip_apart.h): a block within r_spread of the goal a peer holds or
has just been given is no target, so stranded teammates with one view do not all fly the long way to one voxel.

explore_far_team() is both (include/fasterhip_stake.h): explore_far_gain()'s utility inside explore_far_spread()'s passes, and a peer's
goal also takes the unknown voxels of the cube of blocks around it out of every gain of the vehicle, so the second of two stranded
teammates flies to the next-best hall, not to another hole of the same one.

enable_heading() adds the vehicle's yaw: next_goals then also gives yaw and dyaw (getDesiredYaw), a vehicle
that has arrived takes a new goal (set_goals: YAWING, then TRAVELING), and sense(fov=...) looks forward only.

The host restatement every cycle is checked against is fhreplan::Planner (faster_amd/host/replan_stub.hpp);
tests/test_gpu_fleet.py and tests/test_gpu_fleet_views.py compare the two cycle by cycle.
"""
from collections import namedtuple
from operator import attrgetter

import numpy as np

from . import abi, capi


# A frontier chooser, as far as the host layer can tell it from the others.  name: in d_<name>_goals, _mask, _records, _work,
# _<name>_work_key and <name>_records(); method: the public method, in messages; dtype: a record; call: the Map method; stage: the name of
# its launch; view_of: the attribute that holds the all-zero view_of of set_unknown's one grid; stream: whether `call` takes the stream;
# work: the library's workspace-bytes function (None: no workspace) and key: what a workspace is reallocated for (None: its size depends
# on n alone, it is allocated once, with the outputs); skip, labels: whether `call` takes the mask of an earlier chooser and group labels.
_Chooser = namedtuple("_Chooser", "name method dtype call stage view_of stream work key skip labels")
_LATTICE = ("dims", "block", "n_views")


class Fleet:
    """N vehicles, one map, one context.  Buffers are torch tensors on `device`; everything runs on the fleet's own stream."""

    CHOOSERS = {c.name: c for c in (
        _Chooser("explore", "explore", abi.frontier_record_dtype, "frontier_goals_device", "frontier_goals", "d_explore_view_of", False,
                 None, None, False, False),
        _Chooser("reach", "explore_reachable", abi.reach_record_dtype, "reach_goals_device", "reach_goals", "d_reach_view_of", True,
                 None, None, False, False),
        _Chooser("spread", "explore_spread", abi.spread_record_dtype, "spread_goals_device", "spread_goals", "d_reach_view_of", True,
                 "fh_spread_work_bytes", None, False, True),
        _Chooser("gain", "explore_gain", abi.gain_record_dtype, "gain_goals_device", "gain_goals", "d_reach_view_of", True,
                 None, None, False, False),
        _Chooser("team", "explore_team", abi.team_record_dtype, "team_goals_device", "team_goals", "d_reach_view_of", True,
                 "fh_spread_work_bytes", None, False, True),
        _Chooser("sight", "explore_sight", abi.sight_record_dtype, "sight_goals_device", "sight_goals", "d_reach_view_of", True,
                 None, None, False, False),
        _Chooser("bid", "explore_bid", abi.bid_record_dtype, "bid_goals_device", "bid_goals", "d_reach_view_of", True,
                 "fh_bid_work_bytes", None, False, True),
        _Chooser("far", "explore_far", abi.far_record_dtype, "far_goals_device", "far_goals", "d_reach_view_of", True,
                 "fh_far_work_bytes", _LATTICE, True, False),
        _Chooser("far_spread", "explore_far_spread", abi.far_spread_record_dtype, "far_spread_goals_device", "far_spread_goals",
                 "d_reach_view_of", True, "fh_apart_work_bytes", _LATTICE + ("n",), True, True),
        _Chooser("far_gain", "explore_far_gain", abi.far_gain_record_dtype, "far_gain_goals_device", "far_gain_goals", "d_reach_view_of", True,
                 "fh_prospect_work_bytes", _LATTICE, True, False),
        _Chooser("far_team", "explore_far_team", abi.far_team_record_dtype, "far_team_goals_device", "far_team_goals", "d_reach_view_of", True,
                 "fh_stake_work_bytes", _LATTICE + ("n",), True, True),
    )}

    def __init__(self, n, params=None, device=0, n_seg=6, max_poly=3, max_points=32, faces_per_problem=192, max_states=1024, dc=0.01,
                 v_max=5.0, a_max=5.0, j_max=8.0, decomp_radius=0.05, dist_max_vertexes=1.5, local_bbox=(2.0, 2.0, 1.0), z_ground=0.0,
                 search="jps"):
        import torch

        self.torch = torch
        self.n, self.N, self.max_poly, self.mp, self.fpp, self.max_states = int(n), int(n_seg), int(max_poly), int(max_points), int(faces_per_problem), int(max_states)
        self.params = np.array(abi.default_fleet_params() if params is None else params, dtype=abi.fleet_params_dtype).reshape(())
        self.decomp_radius, self.dist_max_vertexes, self.local_bbox, self.z_ground = float(decomp_radius), float(dist_max_vertexes), tuple(local_bbox), float(z_ground)
        self.dev = torch.device("cuda", device)
        self.stream = torch.cuda.Stream(device=self.dev)
        self.ctx, self.map = capi.Context(device), capi.Map(device)
        self.ctx.set_stream(self.stream.cuda_stream)
        self.map.set_stream(self.stream.cuda_stream)
        self.map.set_search(search)
        rule = self.params["rule"]
        self.ctx.set_pair_rule(mode=int(rule["mode"]), r_known=float(rule["r_known"]), drone_radius=float(rule["drone_radius"]),
                               delta_h=float(rule["delta_h"]), delta_a=float(rule["delta_a"]))
        B, u8, i32, f64 = self.n, torch.uint8, torch.int32, torch.float64
        whole = abi.make_problems(B)
        whole["n_seg"], whole["force_final_pos"], whole["dc"] = self.N, 1, dc
        whole["v_max"], whole["a_max"], whole["j_max"] = v_max, a_max, j_max
        safe = whole.copy()
        safe["force_final_pos"] = 0
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.dev)  # noqa: E731
        self.d_vehicles = z(B * abi.vehicle_dtype.itemsize, u8)
        self.d_plans = z(B * self.max_states * abi.state_dtype.itemsize, u8)
        self.d_whole = torch.from_numpy(whole.view(np.uint8).copy()).to(self.dev)
        self.d_safe = torch.from_numpy(safe.view(np.uint8).copy()).to(self.dev)
        self.d_starts, self.d_goals, self.d_radius, self.d_active = z((B, 3), f64), z((B, 3), f64), z(B, f64), z(B, i32)
        self.d_paths, self.d_np, self.d_ex = z((B, self.mp, 3), f64), z(B, i32), z(B, torch.int64)
        FB, RES = abi.face_dtype.itemsize, abi.result_dtype.itemsize
        self.d_wf, self.d_sf = z(B * self.fpp * FB, u8), z(B * self.fpp * FB, u8)
        self.d_off, self.d_npoly, self.d_last = z((B, 9), i32), z(B, i32), z((B, 3), f64)
        self.d_wr, self.d_sr = z(B * RES, u8), z(B * RES, u8)
        self.d_spaths, self.d_snp = z((B, self.max_poly + 1, 3), f64), z(B, i32)
        self.d_next = z(B * abi.state_dtype.itemsize, u8)
        self.cloud, self.n_cloud, self.grid = None, 0, None
        self.flags = self.view_flags = self.view_of = None
        self.n_views = 0
        self.dc = float(dc)
        self.d_headings = self.d_goal_yaw = self.yaw_params = None  # enable_heading
        self.point_mask, self.map_args = None, None                 # set_point_views; what set_map built the map with
        self.traffic_par, self.n_cloud_all = None, 0                # enable_traffic: the cloud holds n_cloud static points, then the traffic
        self.obstacle_par = self.d_obstacles = None                 # enable_obstacles: then the obstacles' points; n_cloud_all is the end
        self.n_obstacles, self.obstacle_tick = 0, 0                 # the obstacle clock: ticks since set_obstacles (next_goals advances it)
        self.track_par = self.d_truth = self.d_tracks = self.d_track_seer = self.d_track_info = None   # enable_tracking
        self.track_los, self.track_tick, self.truth_tick = False, 0, 0   # the sightings' clock; ticks since set_truth (next_goals advances both)
        self.check_par = self.check_cells = self.d_backup_vehicles = self.d_backup_plans = self.d_check = None   # enable_check
        self.round_par = self.round_cells = self.d_rounds = self.d_active_begin = self.d_check_rounds = None      # enable_rounds
        self.round_retries, self.round_fixed = 0, False
        self.listed_views, self._views_full, self.d_view_list, self.d_view_count = False, True, None, None   # enable_listed_views
        self.d_link_labels = self.d_link_info = None                                                           # link
        self.d_coverage = self.d_explore_view_of = self.d_reach_view_of = None   # coverage; set_unknown's one grid as a view: explore, the others
        for ch in self.CHOOSERS.values():   # explore .. explore_far_team: d_<name>_goals, _mask, _records, _work and _<name>_work_key
            for attr in ("d_%s_goals", "d_%s_mask", "d_%s_records") + (("d_%s_work",) if ch.work else ()) + (("_%s_work_key",) if ch.key else ()):
                setattr(self, attr % ch.name, None)
        torch.cuda.synchronize(self.dev)

    def close(self):
        if self.map is not None:
            self.map.close()
            self.ctx.close()
            self.map = self.ctx = None

    def _host_to_device(self, a, dtype):
        t = self.torch
        if isinstance(a, t.Tensor):
            return a.to(self.dev, dtype=dtype).contiguous()
        return t.from_numpy(np.ascontiguousarray(a)).to(self.dev, dtype=dtype)

    def _follow_current(self):
        self.stream.wait_stream(self.torch.cuda.current_stream(self.dev))

    # ---- per-vehicle set-up and per-cycle inputs ----
    def init(self, states, goals):
        """setTerminalGoal(goals[i]) + the first updateState(states[i]) of every vehicle.  states: [n] abi.state_dtype or [n][3] positions."""
        states = np.asarray(states)
        if states.dtype != abi.state_dtype:
            s = np.zeros(self.n, dtype=abi.state_dtype)
            s["pos"] = np.asarray(states, dtype=np.float64).reshape(self.n, 3)
            states = s
        d_states = self._host_to_device(states.view(np.uint8).reshape(-1), self.torch.uint8)
        d_goals = self._host_to_device(np.asarray(goals, dtype=np.float64).reshape(self.n, 3), self.torch.float64)
        self._follow_current()
        with self.torch.cuda.stream(self.stream):
            self.ctx.fleet_init_device(self.params, d_states.data_ptr(), d_goals.data_ptr(), self.n, self.max_states, self.d_vehicles.data_ptr(),
                                       self.d_plans.data_ptr())
            d_states.record_stream(self.stream)
            d_goals.record_stream(self.stream)

    def set_map(self, cloud, cells, res, center, z_max, inflation):
        """This cycle's occupied points (numpy or a device tensor [m][3]): the occupancy grid of the path search (MapUtil::readMap) and the
        obstacles of both corridors.  With traffic enabled these are the static points: they are copied in front of the traffic points,
        which stay, and must end in the same word of the masks as the cloud they replace."""
        static =self._host_to_device(np.asarray(cloud, dtype=np.float64).reshape(-1, 3) if not isinstance(cloud, self.torch.Tensor) else cloud,
                                      self.torch.float64)
        if self._tail_first() is not None:
            # the tail stays: the new static points are copied in front of it, on the fleet's stream (launches in flight read the cloud)
            if abi.point_mask_words(static.shape[0]) * 32 != self._tail_first():
                raise capi.FasterHipError("Fleet.set_map: with traffic enabled the new cloud must end in the same word of the masks (%d points, "
                                          "the traffic begins at %d): set_point_views and enable_traffic again"
                                          % (static.shape[0], self._tail_first()))
            self._follow_current()
            with self.torch.cuda.stream(self.stream):
                self._write_static(self.cloud, static)
                static.record_stream(self.stream)
            self.n_cloud = int(static.shape[0])
        else:
            self.cloud = static
            self.n_cloud = int(self.cloud.shape[0])
        self._follow_current()
        self.cloud.record_stream(self.stream)  # (read by every later cycle's launches on the fleet's stream)
        self.map.read_device(self.cloud.data_ptr(), self.n_cloud, cells, res, center, self.z_ground, z_max, inflation)
        self.map_args = (tuple(int(c) for c in cells), float(res), tuple(float(c) for c in center), float(z_max), float(inflation))
        self._views_changed()
        if self.point_mask is not None and self.point_mask.shape[1] * 32 < self.n_cloud:
            raise capi.FasterHipError("Fleet.set_map: the point masks hold fewer bits than the new cloud has points (set_point_views again)")

    def set_unknown(self, flags, origin, res, dims):
        """This cycle's unknown voxels: flags[(iz ny + iy) nx + ix] != 0 (numpy or a device tensor) on the lattice (origin, res, dims)."""
        self.flags = self._host_to_device(np.asarray(flags, dtype=np.uint8).reshape(-1) if not isinstance(flags, self.torch.Tensor) else flags,
                                          self.torch.uint8)
        self.grid = (tuple(float(o) for o in origin), float(res), tuple(int(d) for d in dims))
        self._follow_current()
        self.flags.record_stream(self.stream)
        self.ctx.set_unknown_grid_device(self.flags.data_ptr(), self.grid[0], self.grid[1], self.grid[2])
        self.view_flags = self.view_of = None  # (one grid replaces views)
        self.n_views = 0
        if self.point_mask is not None:        # (point masks are numbered by views: gone with them)
            self.set_point_views(False)

    def set_unknown_views(self, flags=None, view_of=None, n_views=None, *, origin, res, dims):
        """Unknown voxels per vehicle: vehicle i reads and senses view view_of[i] (None: view i, n_views = n) of a [n_views][cells] uint8
        device tensor, cells = dims[0] dims[1] dims[2], each view laid out like set_unknown's grid.  flags = None allocates the views, all
        ones: everything unknown; a tensor is adopted as it is (not copied when it is already on the device: sense() writes into it).
        Memory: n_views x cells bytes.  Where a view per vehicle does not fit, view_of lets vehicles share views (a team with one map)."""
        t = self.torch
        dims = tuple(int(d) for d in dims)
        cells = dims[0] * dims[1] * dims[2]
        if view_of is not None:
            self.view_of = self._host_to_device(np.asarray(view_of, dtype=np.int32).reshape(-1) if not isinstance(view_of, t.Tensor) else view_of, t.int32)
            if self.view_of.numel() != self.n:
                raise capi.FasterHipError("Fleet.set_unknown_views: view_of needs one entry per vehicle")
        else:
            self.view_of = None
        if flags is None:
            n_views = int(n_views) if n_views is not None else self.n
            self.view_flags = t.ones((n_views, cells), dtype=t.uint8, device=self.dev)
        else:
            f = flags if isinstance(flags, t.Tensor) else np.asarray(flags, dtype=np.uint8)
            self.view_flags = self._host_to_device(f, t.uint8).reshape(-1, cells)
            if n_views is not None and int(n_views) != self.view_flags.shape[0]:
                raise capi.FasterHipError("Fleet.set_unknown_views: flags hold %d views, n_views = %d" % (self.view_flags.shape[0], int(n_views)))
        self.n_views = int(self.view_flags.shape[0])
        if self.view_of is None and self.n_views < self.n:
            raise capi.FasterHipError("Fleet.set_unknown_views: %d views for %d vehicles need view_of" % (self.n_views, self.n))
        if self.view_of is not None and (int(self.view_of.min()) < 0 or int(self.view_of.max()) >= self.n_views):
            raise capi.FasterHipError("Fleet.set_unknown_views: view_of names a view outside [0, %d)" % self.n_views)
        self.grid = (tuple(float(o) for o in origin), float(res), dims)
        self.flags = None
        self._follow_current()
        self.view_flags.record_stream(self.stream)
        if self.view_of is not None:
            self.view_of.record_stream(self.stream)
        self.ctx.set_unknown_views_device(self.view_flags.data_ptr(), cells, None if self.view_of is None else self.view_of.data_ptr(), self.n_views,
                                          self.grid[0], self.grid[1], self.grid[2])
        if self.point_mask is not None:  # (the masks are numbered by the same views: the table that was just replaced must not stay attached)
            if self.point_mask.shape[0] != self.n_views:
                raise capi.FasterHipError("Fleet.set_unknown_views: %d views, the point masks hold %d (set_point_views again)" % (self.n_views, self.point_mask.shape[0]))
            self.ctx.set_point_views_device(self.point_mask.data_ptr(), self.point_mask.shape[1], None if self.view_of is None else self.view_of.data_ptr(),
                                            self.n_views)
        self._views_changed()

    def set_point_views(self, mask=None):
        """Occupied space per view: mask [n_views][ceil(n_cloud / 32)] uint32 (numpy or a device tensor, adopted as it is when it is on the
        device: observe() writes into it), bit k & 31 of word k >> 5 of row v set iff view v knows point k of set_map's cloud.  The views
        are those of set_unknown_views (the same view_of, the same count), which comes first.  mask = None allocates all zeros: nothing is
        known.  From now on replan() rebuilds one occupancy grid per view from the masks ("map_views"), searches every vehicle's path in
        the grid of its view and cuts both corridors around the points its view knows.  mask = False detaches: replan() is what it was.
        Memory per view: a grid of ceil(cells / 32) words and a mask row; the jump point search adds 64 bytes per cell and view."""
        t = self.torch
        if self._tail_first() is not None:   # (traffic and obstacles live in masks that are replaced: enable_traffic, enable_obstacles again)
            self.traffic_par, self.n_cloud_all = None, 0
            self.obstacle_par = self.d_obstacles = None
            self.track_par = self.d_truth = self.d_tracks = self.d_track_seer = self.d_track_info = None
            self.cloud = self.cloud[:self.n_cloud]
        if mask is False:
            self.point_mask = None
            self.listed_views = False   # (no views to list)
            self.ctx.set_point_views_device(None)
            return
        if self.view_flags is None or self.cloud is None:
            raise capi.FasterHipError("Fleet.set_point_views: set_map and set_unknown_views first")
        words = abi.point_mask_words(self.n_cloud)
        if mask is None:
            self.point_mask = t.zeros((self.n_views, words), dtype=t.int32, device=self.dev)
        else:
            m = mask if isinstance(mask, t.Tensor) else t.from_numpy(np.ascontiguousarray(mask, dtype=np.uint32).view(np.int32))
            self.point_mask = m.to(self.dev).view(t.int32).reshape(self.n_views, -1).contiguous()
            if self.point_mask.shape[1] < words:
                raise capi.FasterHipError("Fleet.set_point_views: %d words per view, the cloud needs %d" % (self.point_mask.shape[1], words))
        self._follow_current()
        self.point_mask.record_stream(self.stream)
        self.ctx.set_point_views_device(self.point_mask.data_ptr(), self.point_mask.shape[1], None if self.view_of is None else self.view_of.data_ptr(),
                                        self.n_views)
        self._views_changed()

    def observe(self):
        """Every view learns the cloud points that lie in voxels it knows (fh_fleet_observe_device): after sense(), before replan().  One
        launch on the fleet's stream; bits are only ORed."""
        if self.point_mask is None:
            raise capi.FasterHipError("Fleet.observe: set_point_views first")
        self._follow_current()
        origin, res, dims = self.grid
        self.ctx.fleet_observe_device(origin, res, dims, self.view_flags.data_ptr(), self.view_flags.shape[1],
                                      None if self.view_of is None else self.view_of.data_ptr(), self.n_views, self.cloud.data_ptr(), self.n_cloud,
                                      self.point_mask.data_ptr(), self.point_mask.shape[1])

    @staticmethod
    def _write_static(cloud, static):
        """The static points into the front of an extended cloud; the points up to the next multiple of 32 are copies of a finite point
        (no bit of theirs is ever set)."""
        m = int(static.shape[0])
        cloud[:m] = static
        first = abi.point_mask_words(m) * 32
        if first > m:
            cloud[m:first] = static[0] if m > 0 else 0.0

    def enable_traffic(self, samples, stride, range, hull=None, rule="all", timed=False, window=0, first_instant=None):  # noqa: A002  (the header's word)
        """The vehicles avoid each other (include/fasterhip_traffic.h): from now on traffic() writes `samples` instants of every committed
        plan, `stride` states apart, as points behind the static cloud and shows them, through the point masks, to the vehicles nearer
        than `range`; hull (None: params["rule"]["drone_radius"]; 0: no hull) inflates every sample to seven points.  rule: "all", or
        "yield": vehicle i sees the vehicles below i only.  After set_map, set_unknown_views with a view per vehicle and
        set_point_views.  The cloud tensor grows to pad32(n_static) + n samples pps points and every mask row to as many bits, keeping
        its words; replan() reads the whole cloud, set_map's shared map, observe() and audit() the static points only.  Memory: n rows
        of ceil(n samples pps / 32) words more.
        timed=True matches the plans instant by instant (include/fasterhip_traffic_timed.h): sample s is the instant first_instant +
        s stride (None: max(params["delta_t"] - 1, 0), the start state of the replan), and a sample of another vehicle is shown to
        vehicle i only when i's own committed plan is nearer than `range` to it within `window` samples of the same instant; at most
        abi.FH_TRAFFIC_TIMED_MAX_SAMPLES samples.  With timed=False window and first_instant are ignored."""
        t = self.torch
        if self.obstacle_par is not None:
            raise capi.FasterHipError("Fleet.enable_traffic: traffic first, the obstacles behind it (set_point_views, enable_traffic, enable_obstacles)")
        if self.cloud is None or self.view_flags is None or self.point_mask is None:
            raise capi.FasterHipError("Fleet.enable_traffic: set_map, set_unknown_views and set_point_views first")
        if self.view_of is not None or self.n_views != self.n:
            raise capi.FasterHipError("Fleet.enable_traffic: needs a view per vehicle (set_unknown_views without view_of, n_views = n)")
        rules = {"all": abi.FH_TRAFFIC_ALL, "yield": abi.FH_TRAFFIC_YIELD_TO_LOWER}
        if rule not in rules:
            raise capi.FasterHipError("Fleet.enable_traffic: rule is \"all\" or \"yield\", got %r" % (rule,))
        hull = float(self.params["rule"]["drone_radius"]) if hull is None else float(hull)
        static = self.cloud[:self.n_cloud]
        first = abi.point_mask_words(self.n_cloud) * 32
        if timed:
            if int(samples) > abi.FH_TRAFFIC_TIMED_MAX_SAMPLES:
                raise capi.FasterHipError("Fleet.enable_traffic: timed traffic takes at most %d samples, got %d"
                                          % (abi.FH_TRAFFIC_TIMED_MAX_SAMPLES, int(samples)))
            first_instant = max(int(self.params["delta_t"]) - 1, 0) if first_instant is None else int(first_instant)
            par = abi.default_traffic_timed_params(samples, stride, range, hull, rules[rule], first, first_instant, window)
        else:
            par = abi.default_traffic_params(samples, stride, range, hull, rules[rule], first)
        total = first + self.n * int(samples) * abi.traffic_points_per_sample(hull)
        if int(samples) < 1 or total >= 1 << 31:
            raise capi.FasterHipError("Fleet.enable_traffic: %d samples of %d vehicles do not fit a cloud" % (int(samples), self.n))
        self._follow_current()
        with t.cuda.stream(self.stream):
            cloud = t.zeros((total, 3), dtype=t.float64, device=self.dev)
            self._write_static(cloud, static)
            words = max(abi.point_mask_words(total), int(self.point_mask.shape[1]))
            mask = t.zeros((self.n_views, words), dtype=t.int32, device=self.dev)
            mask[:, :self.point_mask.shape[1]] = self.point_mask
            if first > self.n_cloud:   # the bits of the padding points stay clear
                mask[:, first // 32 - 1] &= (1 << (self.n_cloud & 31)) - 1
            mask[:, first // 32:] = 0
        self.cloud, self.point_mask = cloud, mask
        self.cloud.record_stream(self.stream)
        self.point_mask.record_stream(self.stream)
        self.ctx.set_point_views_device(self.point_mask.data_ptr(), self.point_mask.shape[1], None, self.n_views)
        self.traffic_par, self.n_cloud_all = par, total
        self._views_changed()

    def traffic(self):
        """The committed plans of the other vehicles into the tail of the cloud and into every vehicle's mask row
        (fh_fleet_traffic_device, or fh_fleet_traffic_timed_device after enable_traffic(timed=True)): after observe(), before replan().
        Two launches on the fleet's stream; the traffic words are written whole, so what a vehicle saw of the others last cycle goes."""
        if self.traffic_par is None:
            raise capi.FasterHipError("Fleet.traffic: enable_traffic first")
        self._follow_current()
        self._traffic_launch()

    def _traffic_launch(self):
        timed = self.traffic_par.dtype == abi.traffic_timed_params_dtype
        (self.ctx.fleet_traffic_timed_device if timed else self.ctx.fleet_traffic_device)(
            self.traffic_par, self.d_vehicles.data_ptr(), self.d_plans.data_ptr(), self.n, self.max_states, self.cloud.data_ptr(),
            self.n_cloud_all, self.point_mask.data_ptr(), self.point_mask.shape[1])

    def _tail_first(self):
        """The cloud index at which what traffic() and obstacles() write begins, None without either."""
        if self.traffic_par is not None:
            return int(self.traffic_par["first_point"])
        return None if self.obstacle_par is None else int(self.obstacle_par["first_point"])

    def enable_obstacles(self, obstacles, samples, stride, range, r_detect=0.0, points=7, window=0, first_instant=None):  # noqa: A002  (the header's word)
        """The vehicles avoid things that move and are no fleet member (include/fasterhip_obstacles.h): obstacles is [m]
        abi.obstacle_dtype (abi.make_obstacles), each a ball that flies p0 + v t from now on.  From now on obstacles() writes `samples`
        instants of every obstacle's flight, `stride` states apart from first_instant on (None: max(params["delta_t"] - 1, 0), the start
        state of the replan), as points behind whatever the cloud holds, static points or static points and traffic, and shows a sample
        to vehicle i when i's own committed plan is nearer than range + the obstacle's radius to it within `window` samples of the same
        instant, once i stands nearer than r_detect to where the obstacle is now (0: everything is known).  points: 1, or 7 for a hull
        at the obstacle's radius.  After set_map, set_unknown_views with a view per vehicle, set_point_views and, if wanted,
        enable_traffic.  The cloud tensor and every mask row grow and keep their words; replan() reads the whole cloud.  The obstacle
        clock starts at 0 and next_goals advances it.  Memory: n rows of ceil(m samples points / 32) words more."""
        t = self.torch
        if self.cloud is None or self.view_flags is None or self.point_mask is None:
            raise capi.FasterHipError("Fleet.enable_obstacles: set_map, set_unknown_views and set_point_views first")
        if self.view_of is not None or self.n_views != self.n:
            raise capi.FasterHipError("Fleet.enable_obstacles: needs a view per vehicle (set_unknown_views without view_of, n_views = n)")
        obs = np.ascontiguousarray(obstacles)
        if obs.dtype != abi.obstacle_dtype:
            raise capi.FasterHipError("Fleet.enable_obstacles: obstacles must be abi.obstacle_dtype records (abi.make_obstacles)")
        m = int(obs.size)
        held = self.n_cloud   # the points in front, which stay: the static ones, or those and the traffic's (obstacles of before go)
        if self.traffic_par is not None:
            tp = self.traffic_par
            held = int(tp["first_point"]) + self.n * int(tp["samples"]) * abi.traffic_points_per_sample(tp["hull"])
        first = abi.point_mask_words(held) * 32
        if not 1 <= int(samples) <= abi.FH_OBSTACLE_MAX_SAMPLES or int(points) not in (1, 7):
            raise capi.FasterHipError("Fleet.enable_obstacles: 1 .. %d samples and 1 or 7 points, got %d and %d"
                                      % (abi.FH_OBSTACLE_MAX_SAMPLES, int(samples), int(points)))
        first_instant = max(int(self.params["delta_t"]) - 1, 0) if first_instant is None else int(first_instant)
        par = abi.default_obstacle_params(samples, stride, range, self.dc, r_detect, points, first, first_instant, window)
        total = first + m * int(samples) * int(points)
        if total >= 1 << 31:
            raise capi.FasterHipError("Fleet.enable_obstacles: %d samples of %d obstacles do not fit a cloud" % (int(samples), m))
        self._follow_current()
        with t.cuda.stream(self.stream):
            cloud = t.zeros((total, 3), dtype=t.float64, device=self.dev)
            cloud[:held] = self.cloud[:held]
            if self.traffic_par is None:
                self._write_static(cloud, self.cloud[:held])
            words = max(abi.point_mask_words(total), int(self.point_mask.shape[1]))
            mask = t.zeros((self.n_views, words), dtype=t.int32, device=self.dev)
            mask[:, :self.point_mask.shape[1]] = self.point_mask
            if first > held:   # the bits of the padding points stay clear
                mask[:, first // 32 - 1] &= (1 << (held & 31)) - 1
            mask[:, first // 32:] = 0
            d_obs = t.from_numpy(obs.view(np.uint8).reshape(-1).copy()).to(self.dev)
        self.cloud, self.point_mask, self.d_obstacles = cloud, mask, d_obs
        for d in (self.cloud, self.point_mask, self.d_obstacles):
            d.record_stream(self.stream)
        self.ctx.set_point_views_device(self.point_mask.data_ptr(), self.point_mask.shape[1], None, self.n_views)
        self.obstacle_par, self.n_cloud_all, self.n_obstacles, self.obstacle_tick = par, total, m, 0
        self.track_par = self.d_truth = self.d_tracks = self.d_track_seer = self.d_track_info = None   # (another m: enable_tracking again)
        self._views_changed()

    def set_obstacles(self, obstacles):
        """New records for the same number of obstacles ([m] abi.obstacle_dtype): what a tracker knows now.  The clock starts again at
        0: p0 is where an obstacle is at this call."""
        if self.obstacle_par is None:
            raise capi.FasterHipError("Fleet.set_obstacles: enable_obstacles first")
        obs = np.ascontiguousarray(obstacles)
        if obs.dtype != abi.obstacle_dtype or int(obs.size) != self.n_obstacles:
            raise capi.FasterHipError("Fleet.set_obstacles: %d abi.obstacle_dtype records, as in enable_obstacles" % self.n_obstacles)
        src = self.torch.from_numpy(obs.view(np.uint8).reshape(-1).copy()).to(self.dev)
        self._follow_current()
        with self.torch.cuda.stream(self.stream):
            self.d_obstacles.copy_(src)
            src.record_stream(self.stream)
        self.obstacle_tick = 0

    def obstacles(self):
        """The predicted positions of the obstacles into their part of the cloud and into every vehicle's mask row
        (fh_fleet_obstacles_device): after observe() and traffic(), before replan(), once a cycle, with rounds too.  Three launches on
        the fleet's stream; the words are written whole, so what a vehicle saw of the obstacles last cycle goes."""
        if self.obstacle_par is None:
            raise capi.FasterHipError("Fleet.obstacles: enable_obstacles first")
        self._follow_current()
        self._obstacles_launch()

    def _obstacles_launch(self):
        self.ctx.fleet_obstacles_device(self.obstacle_par, self.d_obstacles.data_ptr(), self.n_obstacles, self.obstacle_tick,
                                        self.d_vehicles.data_ptr(), self.d_plans.data_ptr(), self.n, self.max_states, self.cloud.data_ptr(),
                                        self.n_cloud_all, self.point_mask.data_ptr(), self.point_mask.shape[1])

    def obstacle_audit_device(self, r=None, stride=1, count=0, obstacles=None, tick0=None):
        """obstacle_audit() without the copy to the host: one launch on the fleet's stream; returns the device tensor of [n]
        fh_plan_obstacle_audit records as bytes (asynchronous)."""
        t, B = self.torch, self.n
        par = abi.default_obstacle_audit_params(float(self.params["rule"]["drone_radius"]) if r is None else r, self.dc, stride, count)
        self._follow_current()
        with t.cuda.stream(self.stream):
            if obstacles is None:
                if self.d_obstacles is None:
                    raise capi.FasterHipError("Fleet.obstacle_audit: enable_obstacles first, or pass obstacles")
                d_obs, m = self.d_obstacles, self.n_obstacles
            else:
                obs = np.ascontiguousarray(obstacles)
                if obs.dtype != abi.obstacle_dtype:
                    raise capi.FasterHipError("Fleet.obstacle_audit: obstacles must be abi.obstacle_dtype records (abi.make_obstacles)")
                d_obs, m = t.from_numpy(obs.view(np.uint8).reshape(-1).copy()).to(self.dev), int(obs.size)
                d_obs.record_stream(self.stream)
            d_out = t.empty(B * abi.plan_obstacle_audit_dtype.itemsize, dtype=t.uint8, device=self.dev)  # (the kernel writes every byte of every record)
            self.ctx.fleet_obstacle_audit_device(par, d_obs.data_ptr() if m else None, m, self.obstacle_tick if tick0 is None else int(tick0),
                                                 self.d_vehicles.data_ptr(), self.d_plans.data_ptr(), B, self.max_states, d_out.data_ptr())
        return d_out

    def obstacle_audit(self, r=None, stride=1, count=0, obstacles=None, tick0=None):
        """The committed plans, the states the vehicles fly, against where the obstacles are at the same instants
        (include/fasterhip_obstacles.h): [n] abi.plan_obstacle_audit_dtype with squared distances.  An obstacle hits when the centres
        are nearer than r (None: params["rule"]["drone_radius"]) + its radius.  obstacles, tick0: other records and another clock than
        the fleet's own, for a fleet that was never told of them (the control of an experiment).  count=params["delta_t"] audits the
        states the next replan cannot change.  A measurement: nothing of the fleet is written (synchronises)."""
        return self._host(self.obstacle_audit_device(r, stride, count, obstacles, tick0), abi.plan_obstacle_audit_dtype)

    def _truth_bytes(self, obstacles, where):
        obs = np.ascontiguousarray(obstacles)
        if obs.dtype != abi.obstacle_dtype or int(obs.size) != self.n_obstacles:
            raise capi.FasterHipError("Fleet.%s: %d abi.obstacle_dtype records, as in enable_obstacles" % (where, self.n_obstacles))
        return self.torch.from_numpy(obs.view(np.uint8).reshape(-1).copy()).to(self.dev)

    def enable_tracking(self, truth, r_detect, los=True, fit=4, min_obs=2, max_age=0, gate=0.0, grow=0.0):
        """The fleet estimates the obstacles it avoids from what its vehicles see (include/fasterhip_track.h).  After enable_obstacles,
        with as many records: truth is [m] abi.obstacle_dtype, where the obstacles really are (p0 + v t from now on: a simulation's
        ground truth, or v = 0 and this cycle's detections through set_truth every cycle).  From now on track() writes the records
        obstacles() reads: an obstacle is seen when a vehicle stands nearer than r_detect to it and, with los, no occupied cell of the
        fleet's map lies between (needs set_map); the newest `fit` sightings are fitted, a record is on from min_obs sightings; a track
        unseen for more than max_age ticks is forgotten (0: never), a sighting farther than `gate` from the prediction starts it anew
        (0: no gate), the radius grows by `grow` per second unseen.  The tracks start empty and the records off; the clock of the
        sightings and the truth's clock start at 0 and next_goals advances both.  Memory: 320 bytes per obstacle."""
        t = self.torch
        if self.obstacle_par is None:
            raise capi.FasterHipError("Fleet.enable_tracking: enable_obstacles first")
        src = self._truth_bytes(truth, "enable_tracking")
        par = abi.default_track_params(r_detect, self.dc, fit, min_obs, max_age, gate, grow)
        m = self.n_obstacles
        self._follow_current()
        with t.cuda.stream(self.stream):
            self.d_truth = src.clone()
            self.d_tracks = t.zeros(m * abi.obstacle_track_dtype.itemsize, dtype=t.uint8, device=self.dev)
            self.d_track_seer = t.full((m,), -1, dtype=t.int32, device=self.dev)
            self.d_track_info = t.zeros(4, dtype=t.int64, device=self.dev)
            self.d_obstacles.zero_()   # (nothing is known yet: every record off)
        for d in (src, self.d_truth, self.d_tracks, self.d_track_seer, self.d_track_info):
            d.record_stream(self.stream)
        self.track_par, self.track_los, self.track_tick, self.truth_tick, self.obstacle_tick = par, bool(los), 0, 0, 0

    def set_truth(self, obstacles):
        """New truth for the same number of obstacles ([m] abi.obstacle_dtype), its clock at 0: p0 is where an obstacle is at this
        call.  The tracks and their clock stay."""
        if self.track_par is None:
            raise capi.FasterHipError("Fleet.set_truth: enable_tracking first")
        src = self._truth_bytes(obstacles, "set_truth")
        self._follow_current()
        with self.torch.cuda.stream(self.stream):
            self.d_truth.copy_(src)
            src.record_stream(self.stream)
        self.truth_tick = 0

    def track(self):
        """What the vehicles see of the truth now, into the tracks and from them into the records of obstacles(), in place on the device
        (fh_fleet_obstacle_track_device): after observe() and traffic(), before obstacles(), once a cycle.  A clear and one launch on the
        fleet's stream.  The records say where an obstacle is NOW, so the obstacle clock starts again at 0."""
        if self.track_par is None:
            raise capi.FasterHipError("Fleet.track: enable_tracking first")
        self._follow_current()
        self._track_launch()

    def _track_launch(self):
        p = lambda t: t.data_ptr()  # noqa: E731
        self.ctx.fleet_obstacle_track_device(self.map if self.track_los else None, self.track_par, p(self.d_truth), self.n_obstacles, self.truth_tick,
                                             self.track_tick, p(self.d_vehicles), self.n, p(self.d_tracks), p(self.d_obstacles), p(self.d_track_seer),
                                             p(self.d_track_info))
        self.obstacle_tick = 0

    def track_records(self):
        """(tracks [m] abi.obstacle_track_dtype, estimates [m] abi.obstacle_dtype, seers [m] int32, info [4] int64) of the last track():
        the ring of sightings and this call's flags per obstacle, the records obstacles() reads, the smallest vehicle that saw each or
        -1, and (seen, records on, resets, lost).  Against the truth: obstacle_audit(obstacles=truth, tick0=fleet.truth_tick)
        (synchronises)."""
        if self.track_par is None:
            raise capi.FasterHipError("Fleet.track_records: enable_tracking first")
        self.sync()
        return (self.d_tracks.cpu().numpy().view(abi.obstacle_track_dtype).copy(), self.d_obstacles.cpu().numpy().view(abi.obstacle_dtype).copy(),
                self.d_track_seer.cpu().numpy().copy(), self.d_track_info.cpu().numpy().copy())

    def enable_check(self, r=None, stride=1, count=0, cells=None):
        """Every commit is checked against the other plans and withheld when it conflicts (include/fasterhip_check.h): from now on
        stages() holds `backup` before `commit` and `check` and `revert` after it.  A vehicle whose new trajectory comes nearer than r
        (None: 2 params["rule"]["drone_radius"], where two hulls touch) to what another vehicle flew before this cycle's commit, or to
        what a vehicle with a lower index committed in it, at the same instant, keeps its previous plan, status and windows and has
        stage FH_FLEET_STAGE_CONFLICT.  stride > 1 or count > 0 test fewer instants: cheaper and weaker.  cells = (origin, res, dims)
        is the grid of the broad phase, by default separation_cells(r); no field of a record depends on it.  Works with or without
        views, traffic and heading.  Memory: a second vehicle array and a second plan array (n max_states states), 32 bytes per record."""
        t, B = self.torch, self.n
        par = abi.default_check_params(2.0 * float(self.params["rule"]["drone_radius"]) if r is None else r)
        par["stride"], par["count"] = stride, count
        self.check_cells = self.separation_cells(float(par["r"])) if cells is None else cells
        self._follow_current()
        with t.cuda.stream(self.stream):
            self.d_backup_vehicles = t.zeros(B * abi.vehicle_dtype.itemsize, dtype=t.uint8, device=self.dev)
            self.d_backup_plans = t.zeros(B * self.max_states * abi.state_dtype.itemsize, dtype=t.uint8, device=self.dev)
            self.d_check = t.zeros(B * abi.plan_check_dtype.itemsize, dtype=t.uint8, device=self.dev)
        for d in (self.d_backup_vehicles, self.d_backup_plans, self.d_check):
            d.record_stream(self.stream)
        self.check_par = par
        if self.round_par is not None:
            self._alloc_round_checks()

    def check_records(self):
        """[n] abi.plan_check_dtype: what the last replan()'s check found (synchronises).  FH_CHECK_CONFLICT: the commit was withheld.
        With enable_rounds: per vehicle the record of the last round in which it was a candidate (the last round's record if it never was)."""
        if self.check_par is None:
            raise capi.FasterHipError("Fleet.check_records: enable_check first")
        if self.round_par is not None:
            by_round = self.check_records_by_round()
            out = by_round[-1].copy()
            found = np.zeros(self.n, dtype=bool)
            for rec in by_round[::-1]:
                take = ~found & ((rec["flags"] & abi.FH_CHECK_CANDIDATE) != 0)
                out[take] = rec[take]
                found |= take
            return out
        return self._host(self.d_check, abi.plan_check_dtype)

    def enable_rounds(self, rounds, reach=None, passes=32, stride=1, count=0, retries=0, classes=None, cells=None):
        """A replan runs in `rounds` priority rounds (include/fasterhip_rounds.h): from now on stages() is
            begin -> round_classes -> for r in 0 .. rounds - 1: gate@r -> [traffic@r] -> [map_views@r] -> path_search@r -> ... ->
            safe_solve@r -> [backup@r] -> commit@r -> [check@r -> revert@r]; the same body `retries` times as @retry t; -> gate_restore.
        begin writes who replans into a buffer of its own; round_classes gives every vehicle a class such that two vehicles whose
        committed plans come nearer than `reach` (None: the traffic's range if traffic is enabled, else 4 params["rule"]["drone_radius"])
        at one tested instant (stride, count as in enable_check) get different classes below the last (greedy colouring in index order,
        settled in `passes` passes: round_records()); gate@r switches the vehicles of class r on and all others off, gate@retry t the
        vehicles whose commit the check took back (retries > 0 needs enable_check first), gate_restore everyone begin had switched on.
        With traffic enabled the traffic stage runs inside every round, so a round sees the plans the earlier rounds committed;
        traffic() before replan() stays legal and is harmless.  With the check enabled every round is backed up, checked against the
        plans as the earlier rounds left them and reverted on its own; the records of all rounds are check_records_by_round().
        classes: an [n] int32 array or tensor fixes the classes (0 <= class < rounds): round_classes is then not launched and the
        records carry the given class with decided_pass = 0.  cells = (origin, res, dims): the grid of the broad phase, by default
        separation_cells(reach); no field of a record depends on it.
        LIMITS.  results(), faces() and certify() describe every vehicle's buffers as the LAST round left them: a vehicle of an earlier
        round then shows an inactive query (its plan and record are what its own round committed).  With point views map_views runs once
        per round for every view, so a cycle costs about `rounds + retries` times the path search and the views' maps; the active
        vehicles of a round are not compacted, and only enable_listed_views rebuilds the views of a round alone.  Rounds change nothing about who a vehicle sees unless
        traffic or the check is enabled: without them every round plans as if alone, and the result is that of one round.
        Memory: 16 bytes per vehicle, n ints, and with the check 32 bytes per vehicle and round."""
        t, B = self.torch, self.n
        rounds, retries = int(rounds), int(retries)
        if not 1 <= rounds <= abi.FH_ROUNDS_MAX:
            raise capi.FasterHipError("Fleet.enable_rounds: 1 <= rounds <= %d, got %d" % (abi.FH_ROUNDS_MAX, rounds))
        if retries < 0 or (retries > 0 and self.check_par is None):
            raise capi.FasterHipError("Fleet.enable_rounds: retries > 0 replan what the check withheld: enable_check first")
        if reach is None:
            reach = float(self.traffic_par["range"]) if self.traffic_par is not None else 4.0 * float(self.params["rule"]["drone_radius"])
        par = abi.default_round_params(reach, rounds)
        par["passes"], par["stride"], par["count"] = passes, stride, count
        self.round_cells = self.separation_cells(float(par["reach"])) if cells is None else cells
        records = None
        if classes is not None:
            cls = classes.cpu().numpy() if isinstance(classes, t.Tensor) else np.asarray(classes)
            cls = cls.astype(np.int32).reshape(-1)
            if cls.size != B or (B and (cls.min() < 0 or cls.max() >= rounds)):
                raise capi.FasterHipError("Fleet.enable_rounds: classes needs one class in [0, %d) per vehicle" % rounds)
            records = np.zeros(B, dtype=abi.plan_round_dtype)
            records["round_class"] = cls
        self._follow_current()
        with t.cuda.stream(self.stream):
            self.d_active_begin = t.zeros(B, dtype=t.int32, device=self.dev)
            if records is None:
                self.d_rounds = t.zeros(B * abi.plan_round_dtype.itemsize, dtype=t.uint8, device=self.dev)
            else:
                self.d_rounds = t.from_numpy(records.view(np.uint8).copy()).to(self.dev)
        for d in (self.d_active_begin, self.d_rounds):
            d.record_stream(self.stream)
        self.round_par, self.round_retries, self.round_fixed = par, retries, records is not None
        if self.check_par is not None:
            self._alloc_round_checks()
        self._views_changed()

    def enable_listed_views(self, on=True):
        """map_views rebuilds only the views that somebody searches (include/fasterhip_view_subset.h): from now on stages() holds, in
        place of map_views, `view_list` — the views of the vehicles that are switched on (d_active as begin or the round's gate left
        it, through view_of), listed on the device, ascending — and a `map_views` that clears, marks and tables the listed views only;
        with rounds one view_list@r and one listed map_views@r per round and retry.  The grid and the tables of a view that is not
        listed stay as they were: the search of that round reads them for no query, and the round that does search the view lists it
        and rebuilds it first, from the cloud and the masks as they stand then.  The lattice is the one thing the argument does not
        cover, so the first map_views after this call, set_map, set_unknown_views, set_point_views, enable_traffic or enable_rounds
        reads every view (Map.read_views_device); what a launch does is decided when it runs.  Needs point views (set_point_views or
        enable_traffic).  on=False: today's chain.  view_lists() reads the lists back.  Memory: n_views + 1 ints per round."""
        if not on:
            self.listed_views = False
            return
        if self.point_mask is None:
            raise capi.FasterHipError("Fleet.enable_listed_views: the fleet has no point views (set_point_views or enable_traffic first)")
        self.listed_views = True
        self._views_changed()

    def _views_changed(self):
        """The next map_views reads every view; the lists have a row per round and retry and an entry per view."""
        self._views_full = True
        if not self.listed_views:
            return
        t = self.torch
        rows = 1 if self.round_par is None else int(self.round_par["rounds"]) + self.round_retries
        if self.d_view_list is None or tuple(self.d_view_list.shape) != (rows, self.n_views):
            self._follow_current()
            with t.cuda.stream(self.stream):
                self.d_view_list = t.full((rows, self.n_views), -1, dtype=t.int32, device=self.dev)
                self.d_view_count = t.zeros(rows, dtype=t.int32, device=self.dev)
            for d in (self.d_view_list, self.d_view_count):
                d.record_stream(self.stream)

    def view_lists(self):
        """(lists [rows][n_views] int32, counts [rows] int32): the views every round (and retry) of the last replan() listed, ascending
        with -1 behind them, and how many; without rounds one row (synchronises)."""
        if not self.listed_views:
            raise capi.FasterHipError("Fleet.view_lists: enable_listed_views first")
        self.sync()
        return self.d_view_list.cpu().numpy().copy(), self.d_view_count.cpu().numpy().copy()

    def _alloc_round_checks(self):
        """The check records of every round: [rounds + retries][n] fh_plan_check."""
        t = self.torch
        rows = int(self.round_par["rounds"]) + self.round_retries
        self._follow_current()
        with t.cuda.stream(self.stream):
            self.d_check_rounds = t.zeros((rows, self.n * abi.plan_check_dtype.itemsize), dtype=t.uint8, device=self.dev)
        self.d_check_rounds.record_stream(self.stream)

    def round_records(self):
        """[n] abi.plan_round_dtype: the class of every vehicle in the last replan(), the pass that decided it, its lower neighbours and
        flags (synchronises); with fixed classes the given ones."""
        if self.round_par is None:
            raise capi.FasterHipError("Fleet.round_records: enable_rounds first")
        return self._host(self.d_rounds, abi.plan_round_dtype)

    def check_records_by_round(self):
        """[rounds + retries][n] abi.plan_check_dtype: what the check of every round of the last replan() found, the retries behind
        the rounds (synchronises)."""
        if self.round_par is None or self.check_par is None:
            raise capi.FasterHipError("Fleet.check_records_by_round: enable_rounds and enable_check first")
        self.sync()
        return self.d_check_rounds.cpu().numpy().view(abi.plan_check_dtype).copy()

    def link(self, range, passes=None, cells=None, los=False):  # noqa: A002  (the header's word)
        """The vehicles nearer than `range` to each other pool what their views know (include/fasterhip_link.h): link_groups labels
        every view with the smallest view of its connected group (`passes` passes of hook and jump, None:
        abi.FH_LINK_DEFAULT_PASSES; link_records() tells whether they settled), link_merge makes the views of a group equal: a voxel is
        known to all when one of them knows it, and with point views so is a point of the static cloud.  The traffic words of the
        masks are per observer and stay as they are.  After sense() and observe(), before replan(); needs set_unknown_views.  cells =
        (origin, res, dims): the grid of the broad phase, by default separation_cells(range); no output byte depends on it.  Launches on
        the fleet's stream.  Nothing is forgotten when the vehicles part.  Memory: n_views ints and four words.
        los=True: walls block a link (include/fasterhip_link_los.h): a pair in range is linked only when no half-cell sample of the ray
        between the two vehicles lies in an occupied cell of the fleet's map other than the cells they stand in; a blocked pair can still
        be one group through a vehicle that sees both.  Needs set_map.  los=False launches exactly what it always has."""
        self._follow_current()
        for _, launch in self.link_stages(range, passes, cells, los):
            launch()

    def link_stages(self, range, passes=None, cells=None, los=False):  # noqa: A002
        """The two launches of link(), in order: [(name, callable)] (scripts/fleet_cycle.py times them one by one); with los=True the
        first is ("link_groups_los", ...) on the fleet's map."""
        t = self.torch
        if self.view_flags is None:
            raise capi.FasterHipError("Fleet.link: set_unknown_views first")
        if los and self.cloud is None:
            raise capi.FasterHipError("Fleet.link: los=True needs set_map")
        par = abi.default_link_params(range)
        if passes is not None:
            par["passes"] = passes
        if cells is None:
            cells = self.separation_cells(float(par["range"]))
        if self.d_link_labels is None or self.d_link_labels.numel() != self.n_views:
            self._follow_current()
            with t.cuda.stream(self.stream):
                self.d_link_labels = t.zeros(self.n_views, dtype=t.int32, device=self.dev)
                self.d_link_info = t.zeros(4, dtype=t.int64, device=self.dev)
            for d in (self.d_link_labels, self.d_link_info):
                d.record_stream(self.stream)
        c, p = self.ctx, (lambda t: t.data_ptr())
        vo = None if self.view_of is None else p(self.view_of)
        mask = None if self.point_mask is None else p(self.point_mask)
        words = 0 if self.point_mask is None else int(self.point_mask.shape[1])
        shared = words if self._tail_first() is None else self._tail_first() // 32   # (below the traffic and the obstacles)
        groups = ("link_groups", lambda: c.fleet_link_groups_device(par, p(self.d_vehicles), self.n, vo, self.n_views, cells,
                                                                    p(self.d_link_labels), p(self.d_link_info)))
        if los:
            groups = ("link_groups_los", lambda: c.fleet_link_groups_los_device(self.map, par, p(self.d_vehicles), self.n, vo, self.n_views, cells,
                                                                                p(self.d_link_labels), p(self.d_link_info)))
        return [
            groups,
            ("link_merge", lambda: c.fleet_link_merge_device(p(self.d_link_labels), self.n_views, p(self.view_flags), self.view_flags.shape[1],
                                                             self.view_flags.shape[1], mask, words, shared)),
        ]

    def link_records(self):
        """(labels [n_views] int32, info [4] int64) of the last link(): the label of every view; the views whose label the last pass
        changed (0: settled), the roots, the linked pairs of vehicles, and info[3]: 0 after link(), after link(los=True) the pairs in
        range that a wall blocks (synchronises)."""
        if self.d_link_labels is None:
            raise capi.FasterHipError("Fleet.link_records: link first")
        self.sync()
        return self.d_link_labels.cpu().numpy().copy(), self.d_link_info.cpu().numpy().copy()

    _EXPLORE_WANT = {"reached": abi.FH_FRONTIER_WANT_REACHED, "no_path": abi.FH_FRONTIER_WANT_NO_PATH, "all": abi.FH_FRONTIER_WANT_ALL}
    _FAR_AFTER = {"explore": "d_explore_mask", "reachable": "d_reach_mask", "spread": "d_spread_mask", "gain": "d_gain_mask",
                  "sight": "d_sight_mask", "team": "d_team_mask", "bid": "d_bid_mask"}

    # ---- what the frontier choosers share (CHOOSERS above says where they differ) ----
    def _zeros(self, specs):
        """A zeroed device tensor per (shape, name of the dtype), allocated on the fleet's stream, which is then recorded on each."""
        t = self.torch
        self._follow_current()
        with t.cuda.stream(self.stream):
            made = [t.zeros(shape, dtype=getattr(t, dtype), device=self.dev) for shape, dtype in specs]
        for d in made:
            d.record_stream(self.stream)
        return made

    def _chooser_views(self, who, view_of):
        """(flags tensor, view_stride, view_of pointer or None, n_views) of the choosers' entry points: the views, or set_unknown's one
        grid as a single view that every vehicle reads (an all-zero view_of, kept in the attribute `view_of` names)."""
        if self.view_flags is not None:
            return self.view_flags, int(self.view_flags.shape[1]), (None if self.view_of is None else self.view_of.data_ptr()), self.n_views
        if self.flags is None:
            raise capi.FasterHipError("Fleet.%s: set_unknown_views (or set_unknown) first" % who)
        if getattr(self, view_of) is None:
            setattr(self, view_of, self._zeros([(self.n, "int32")])[0])
        return self.flags, int(self.flags.numel()), getattr(self, view_of).data_ptr(), 1

    def _explore_views(self):
        return self._chooser_views("explore", "d_explore_view_of")

    def _chooser_inputs(self, ch, par, r_avoid, z, want, max_hops=None):
        """What the choosers share before anything is allocated: the preconditions, raised in the name of the chooser's method; the
        views (_chooser_views); and the fields that all their params have in common, written into `par` (max_hops: but for
        fh_frontier_params)."""
        if self.cloud is None or self.map_args is None:
            raise capi.FasterHipError("Fleet.%s: set_map first" % ch.method)
        views = self._chooser_views(ch.method, ch.view_of)
        wants = (want,) if isinstance(want, str) else tuple(want)
        if not wants or any(w not in self._EXPLORE_WANT for w in wants):
            raise capi.FasterHipError("Fleet.%s: want is \"reached\", \"no_path\", \"all\" or a tuple of them, got %r" % (ch.method, want))
        if "reached" in wants and self.d_headings is None:
            raise capi.FasterHipError("Fleet.%s: want=\"reached\" needs enable_heading first (a vehicle that takes a new goal "
                                      "after GOAL_REACHED is YAWING until next_goals with headings has turned it)" % ch.method)
        par["r_avoid"] = float(self.params["goal_radius"]) if r_avoid is None else r_avoid
        par["z_lo"], par["z_hi"] = (self.z_ground, self.map_args[3]) if z is None else z
        par["want"] = 0
        for w in wants:
            par["want"] |= self._EXPLORE_WANT[w]
        if max_hops is not None:
            par["max_hops"] = max_hops
        return views

    def _check_groups(self, ch, groups):
        if groups not in ("link", "view"):
            raise capi.FasterHipError("Fleet.%s: groups is \"link\" or \"view\", got %r" % (ch.method, groups))

    def _far_skip(self, ch, after):
        """The mask of the chooser `after` names (None: nobody is skipped)."""
        if after is None:
            return None
        if after not in self._FAR_AFTER:
            raise capi.FasterHipError("Fleet.%s: after is None or one of %s, got %r" % (ch.method, ", ".join(sorted(self._FAR_AFTER)), after))
        skip = getattr(self, self._FAR_AFTER[after])
        if skip is None:
            raise capi.FasterHipError("Fleet.%s: after=%r, but that chooser has not run" % (ch.method, after))
        return skip

    def _far_work_bytes(self, ch, block, n_views, max_words):
        """The bytes of a far chooser's workspace on the fleet's lattice; 0 from the library is a block it refuses."""
        g = capi._grid_record(self.grid)
        args = (abi.ptr(g), int(block), int(n_views)) + ((int(self.n),) if "n" in ch.key else ())
        work_bytes = int(getattr(capi.lib(), ch.work)(*args))
        if work_bytes == 0:
            raise capi.FasterHipError("Fleet.%s: block must be 1 .. 16 and the blocks of the lattice must fit %d words of 64 "
                                      "(got block %r on a lattice of %s)" % (ch.method, max_words, block, tuple(int(d) for d in self.grid[2])))
        return work_bytes

    def _chooser_buffers(self, ch, n_views, work_bytes, block):
        """Goals, mask and records of a chooser, allocated once; a workspace without a key with them; a workspace with a key whenever
        the key (the lattice, the block, the number of views and, for a team, of vehicles) is not the one it was allocated for."""
        goals, mask, records, work = ("d_%s_%s" % (ch.name, w) for w in ("goals", "mask", "records", "work"))
        if getattr(self, goals) is None:
            names = [goals, mask, records] + ([work] if ch.work and not ch.key else [])
            specs = [((self.n, 3), "float64"), (self.n, "int32"), (self.n * ch.dtype.itemsize, "uint8"), (work_bytes, "uint8")]
            for name, d in zip(names, self._zeros(specs[:len(names)])):
                setattr(self, name, d)
        if ch.key:
            key = (tuple(int(d) for d in self.grid[2]), int(block), int(n_views)) + ((int(self.n),) if "n" in ch.key else ())
            if getattr(self, "_%s_work_key" % ch.name) != key:
                setattr(self, work, self._zeros([(work_bytes, "uint8")])[0])
                setattr(self, "_%s_work_key" % ch.name, key)

    def _chooser_stages(self, ch, par, views, work_bytes=None, block=None, skip=None, groups=None):
        """The two launches of a chooser, in order: [(stage, callable), ("set_goals", callable)].  Allocates what is missing; the
        launches read the fleet's buffers when they run."""
        flags, stride, vo, n_views = views
        if ch.work and not ch.key:
            work_bytes = int(getattr(capi.lib(), ch.work)(self.n))
        self._chooser_buffers(ch, n_views, work_bytes, block)
        # the labels are per view: with set_unknown's single view there is nothing to label
        labels = self.d_link_labels if ch.labels and groups == "link" and self.view_flags is not None and self.d_link_labels is not None \
            and self.d_link_labels.numel() == n_views else None
        goals, mask, records, work = ("d_%s_%s" % (ch.name, w) for w in ("goals", "mask", "records", "work"))
        # what a launch does is what the host pays per period: the methods are bound here, the fleet's own buffers are fetched in one
        # attrgetter when the launch runs, and the pointers of `skip` and `labels` (None: a null pointer) are asked for then, too
        call, set_goals = getattr(self.map, ch.call), self.ctx.fleet_set_goals_device
        fetch, chosen = attrgetter("d_vehicles", *([work] if ch.work else []), goals, mask, records), attrgetter("d_vehicles", goals, mask)
        if ch.work:   # (a workspace comes with skip, labels or both, and with the stream)
            takes_skip, takes_labels = ch.skip, ch.labels
            skip_ptr, labels_ptr = (x if x is None else x.data_ptr for x in (skip, labels))

            def choose():
                v, w, g, k, r = fetch(self)
                call(par, self.grid, flags.data_ptr(), stride, vo, n_views, *((skip_ptr and skip_ptr(),) if takes_skip else ()),
                     *((labels_ptr and labels_ptr(),) if takes_labels else ()), v.data_ptr(), self.n, w.data_ptr(), work_bytes, g.data_ptr(),
                     k.data_ptr(), r.data_ptr(), self.stream.cuda_stream)
        else:
            stream = (lambda: (self.stream.cuda_stream,)) if ch.stream else tuple   # (frontier_goals_device: the map's own stream)

            def choose():
                v, g, k, r = fetch(self)
                call(par, self.grid, flags.data_ptr(), stride, vo, n_views, v.data_ptr(), self.n, g.data_ptr(), k.data_ptr(), r.data_ptr(), *stream())

        def apply():
            v, g, k = chosen(self)
            set_goals(self.params, v.data_ptr(), g.data_ptr(), k.data_ptr(), self.n)

        return [(ch.stage, choose), ("set_goals", apply)]

    def _run(self, stages):
        self._follow_current()
        for _, launch in stages:
            launch()

    def _chooser_records(self, ch):
        """(records [n] ch.dtype, goals [n][3], mask [n] int32) of the chooser's last run (synchronises)."""
        goals = getattr(self, "d_%s_goals" % ch.name)
        if goals is None:
            raise capi.FasterHipError("Fleet.%s_records: %s first" % (ch.name, ch.method))
        self.sync()
        return (getattr(self, "d_%s_records" % ch.name).cpu().numpy().view(ch.dtype).copy(), goals.cpu().numpy().copy(),
                getattr(self, "d_%s_mask" % ch.name).cpu().numpy().copy())

    def explore(self, r_max, r_avoid=None, z=None, want="reached"):
        """The wanted vehicles take the nearest frontier voxel of their view as terminal goal (include/fasterhip_frontier.h): a voxel the
        view knows, free in the map, nearer than r_max, with an unknown face neighbour.  want: "reached" (status GOAL_REACHED), "no_path"
        (the last replan found no path), "all", or a tuple of them.  r_avoid: no voxel nearer than this to the goal the vehicle has (None:
        params["goal_radius"]); z = (z_lo, z_hi) of the voxel centres, both inclusive (None: z_ground and the z_max of set_map).  Two
        launches on the fleet's stream: frontier_goals into buffers of the fleet (explore_records()), then fh_fleet_set_goals_device with
        that mask; a vehicle without a candidate keeps goal and status.  After sense(), observe() and link(), before replan(); needs
        set_map and set_unknown_views (set_unknown's one grid counts as a single view of all vehicles), and, for "reached",
        enable_heading: a vehicle that set_goals made YAWING leaves that status only in next_goals with headings."""
        self._run(self.explore_stages(r_max, r_avoid, z, want))   # (raises before anything is launched)

    def explore_stages(self, r_max, r_avoid=None, z=None, want="reached"):
        """The two launches of explore(), in order: [(name, callable)] (scripts/fleet_cycle.py times them one by one)."""
        ch = self.CHOOSERS["explore"]
        par = abi.default_frontier_params(r_max)
        return self._chooser_stages(ch, par, self._chooser_inputs(ch, par, r_avoid, z, want))

    def explore_records(self):
        """(records [n] abi.frontier_record_dtype, goals [n][3], mask [n] int32) of the last explore() (synchronises)."""
        return self._chooser_records(self.CHOOSERS["explore"])

    def explore_reachable(self, r_max, r_avoid=None, z=None, want="reached", max_hops=0):
        """explore() with the choice of include/fasterhip_reach.h: of the frontier voxels of explore() the one that a flood of the space
        the view knows to be free, from the voxel the vehicle stands in and over the box of its sphere, reaches in the fewest steps (six
        neighbours; then the smallest distance), and never one the flood does not reach: a voxel behind a wall or in a sealed pocket is
        not chosen, so the replan that follows is not spent on NO_PATH.  max_hops: the last level of the flood, 0 for no limit.  The
        other arguments, the preconditions and the two launches are those of explore(); the buffers are its own (reach_records())."""
        self._run(self.explore_reachable_stages(r_max, r_avoid, z, want, max_hops))   # (raises before anything is launched)

    def explore_reachable_stages(self, r_max, r_avoid=None, z=None, want="reached", max_hops=0):
        """The two launches of explore_reachable(), in order: [(name, callable)] (scripts/fleet_cycle.py times them one by one)."""
        ch = self.CHOOSERS["reach"]
        par = abi.default_reach_params(r_max)
        return self._chooser_stages(ch, par, self._chooser_inputs(ch, par, r_avoid, z, want, max_hops))

    def reach_records(self):
        """(records [n] abi.reach_record_dtype, goals [n][3], mask [n] int32) of the last explore_reachable() (synchronises)."""
        return self._chooser_records(self.CHOOSERS["reach"])

    def explore_far(self, block=8, r_avoid=None, z=None, want="reached", max_hops=0, after=None):
        """The fallback behind the other choosers (include/fasterhip_far.h): a wanted vehicle takes the nearest frontier voxel of its
        WHOLE view that a flood over blocks of block x block x block voxels reaches from the block it stands in — two blocks are joined
        where a pair of free voxels touches across the face they share — the fewest block steps first, then the nearest block, and in
        it the nearest frontier voxel.  after: the chooser that ran earlier in this period, "explore", "reachable", "spread", "gain",
        "sight", "team" or "bid"; the vehicles it gave a goal are skipped (None: nobody is).  block: 1 .. 16, and the blocks of the
        lattice must fit abi.FH_FAR_MAX_WORDS words of 64.  max_hops: the last level of the flood, 0 for no limit.  The other arguments,
        the preconditions and the errors are those of explore_reachable(); the buffers and the workspace are its own (far_records())."""
        self._run(self.explore_far_stages(block, r_avoid, z, want, max_hops, after))   # (raises before anything is launched)

    def explore_far_stages(self, block=8, r_avoid=None, z=None, want="reached", max_hops=0, after=None):
        """The two launches of explore_far(), in order: [(name, callable)] (scripts/fleet_cycle.py times them one by one)."""
        ch = self.CHOOSERS["far"]
        par = abi.default_far_params(block)
        views = self._chooser_inputs(ch, par, r_avoid, z, want, max_hops)
        skip = self._far_skip(ch, after)
        work_bytes = self._far_work_bytes(ch, block, views[3], abi.FH_FAR_MAX_WORDS)
        return self._chooser_stages(ch, par, views, work_bytes, block, skip)

    def far_records(self):
        """(records [n] abi.far_record_dtype, goals [n][3], mask [n] int32) of the last explore_far() (synchronises)."""
        return self._chooser_records(self.CHOOSERS["far"])

    def explore_far_gain(self, block=8, gain_blocks=2, hop_cost=None, min_gain=0, r_avoid=None, z=None, want="reached", max_hops=0, after=None):
        """explore_far() with a gain (include/fasterhip_prospect.h): every block of the flood carries the number of its unknown voxels,
        the gain of a target block is the sum of those numbers over the cube of 2 gain_blocks - 1 blocks an edge around it (0 .. 5
        blocks; 0: every gain is 0), and of the target blocks of ALL levels the one with the largest  gain - hop_cost * hops  is taken
        (then the fewest block steps, the nearest block, and in it explore_far()'s voxel), so the edge of an unexplored hall three
        blocks on beats a one-voxel hole next door.  hop_cost: the unknown voxels a block step must be worth, 0 .. 16384; None means
        block * block, the voxels of one face of a block — a judgement, not a measurement.  min_gain: a target block with a smaller
        gain is poor and never taken (abi.FH_PROSPECT_ALL_POOR where every reachable one is).  after, block and the other arguments,
        the preconditions and the errors are explore_far()'s; the buffers and the workspace are its own (far_gain_records())."""
        self._run(self.explore_far_gain_stages(block, gain_blocks, hop_cost, min_gain, r_avoid, z, want, max_hops, after))   # (raises before anything is launched)

    def explore_far_gain_stages(self, block=8, gain_blocks=2, hop_cost=None, min_gain=0, r_avoid=None, z=None, want="reached", max_hops=0,
                                after=None):
        """The two launches of explore_far_gain(), in order: [(name, callable)] (scripts/fleet_cycle.py times them one by one)."""
        ch = self.CHOOSERS["far_gain"]
        par = abi.default_far_gain_params(block, gain_blocks)
        views = self._chooser_inputs(ch, par, r_avoid, z, want, max_hops)
        skip = self._far_skip(ch, after)
        work_bytes = self._far_work_bytes(ch, block, views[3], abi.FH_PROSPECT_MAX_WORDS)
        if not 0 <= int(gain_blocks) <= abi.FH_PROSPECT_MAX_BLOCKS:
            raise capi.FasterHipError("Fleet.explore_far_gain: gain_blocks must be 0 .. %d, got %r" % (abi.FH_PROSPECT_MAX_BLOCKS, gain_blocks))
        if hop_cost is not None:
            if not 0 <= int(hop_cost) <= abi.FH_PROSPECT_MAX_HOP_COST:
                raise capi.FasterHipError("Fleet.explore_far_gain: hop_cost must be None or 0 .. %d, got %r" % (abi.FH_PROSPECT_MAX_HOP_COST, hop_cost))
            par["hop_cost"] = int(hop_cost)
        if int(min_gain) < 0:
            raise capi.FasterHipError("Fleet.explore_far_gain: min_gain must be >= 0, got %r" % (min_gain,))
        par["min_gain"] = int(min_gain)
        return self._chooser_stages(ch, par, views, work_bytes, block, skip)

    def far_gain_records(self):
        """(records [n] abi.far_gain_record_dtype, goals [n][3], mask [n] int32) of the last explore_far_gain() (synchronises)."""
        return self._chooser_records(self.CHOOSERS["far_gain"])

    def explore_far_spread(self, block=8, r_spread=2.0, r_avoid=None, z=None, want="reached", max_hops=0, passes=None, groups="link", after=None):
        """explore_far() for a team (include/fasterhip_apart.h): a block of the flood nearer than r_spread to the goal that a peer
        is on its way to, or that a peer with a lower index has been given by an earlier pass of this call, is no target, so stranded
        teammates with one view fly to different far frontiers.  A vehicle that `after`'s chooser gave a goal is skipped and claims
        that goal.  groups and passes are explore_spread()'s (no list, so no overflow; a vehicle with `passes` searching peers below
        it is FH_APART_UNSETTLED for a period); after, block and the other arguments are explore_far()'s; the buffers and the
        workspace are its own (far_spread_records())."""
        self._run(self.explore_far_spread_stages(block, r_spread, r_avoid, z, want, max_hops, passes, groups, after))   # (raises before anything is launched)

    def explore_far_spread_stages(self, block=8, r_spread=2.0, r_avoid=None, z=None, want="reached", max_hops=0, passes=None, groups="link",
                                  after=None):
        """The launches of explore_far_spread(), in order: [(name, callable)], set_goals last (scripts/fleet_cycle.py times them)."""
        ch = self.CHOOSERS["far_spread"]
        self._check_groups(ch, groups)
        par = abi.default_far_spread_params(block, r_spread)
        views = self._chooser_inputs(ch, par, r_avoid, z, want, max_hops)
        if passes is not None:
            par["passes"] = passes
        skip = self._far_skip(ch, after)
        work_bytes = self._far_work_bytes(ch, block, views[3], abi.FH_FAR_MAX_WORDS)
        return self._chooser_stages(ch, par, views, work_bytes, block, skip, groups)

    def far_spread_records(self):
        """(records [n] abi.far_spread_record_dtype, goals [n][3], mask [n] int32) of the last explore_far_spread() (synchronises)."""
        return self._chooser_records(self.CHOOSERS["far_spread"])

    def explore_far_team(self, block=8, r_spread=2.0, gain_blocks=2, hop_cost=None, min_gain=0, claim_blocks=None, r_avoid=None, z=None,
                         want="reached", max_hops=0, passes=None, groups="link", after=None):
        """explore_far_gain() inside the passes of explore_far_spread() (include/fasterhip_stake.h): a target block is weighed by the
        unknown voxels of the cube of 2 gain_blocks - 1 blocks around it, the best  gain - hop_cost * hops  of all levels is taken,
        and the goal a peer is on its way to, or that a peer with a lower index has been given by an earlier pass of this call, removes
        the target blocks within r_spread of it AND, from every gain of the vehicle, the unknown voxels of the cube of
        2 claim_blocks - 1 blocks around its block (0 .. 5; None means gain_blocks; 0: nothing is covered): that peer uncovers them
        anyway.  gain_blocks, hop_cost and min_gain are explore_far_gain()'s, r_spread, passes, groups and after
        explore_far_spread()'s, whose errors are raised before anything is launched; the buffers and the workspace are its own
        (far_team_records())."""
        self._run(self.explore_far_team_stages(block, r_spread, gain_blocks, hop_cost, min_gain, claim_blocks, r_avoid, z, want, max_hops, passes,
                                               groups, after))   # (raises before anything is launched)

    def explore_far_team_stages(self, block=8, r_spread=2.0, gain_blocks=2, hop_cost=None, min_gain=0, claim_blocks=None, r_avoid=None, z=None,
                                want="reached", max_hops=0, passes=None, groups="link", after=None):
        """The launches of explore_far_team(), in order: [(name, callable)], set_goals last (scripts/fleet_cycle.py times them)."""
        ch = self.CHOOSERS["far_team"]
        self._check_groups(ch, groups)
        par = abi.default_far_team_params(block, r_spread, gain_blocks)
        views = self._chooser_inputs(ch, par, r_avoid, z, want, max_hops)
        if not (np.isfinite(float(r_spread)) and float(r_spread) > 0.0):
            raise capi.FasterHipError("Fleet.explore_far_team: r_spread must be finite and > 0, got %r" % (r_spread,))
        if passes is not None:
            if not 1 <= int(passes) <= abi.FH_STAKE_MAX_PASSES:
                raise capi.FasterHipError("Fleet.explore_far_team: passes must be None or 1 .. %d, got %r" % (abi.FH_STAKE_MAX_PASSES, passes))
            par["passes"] = int(passes)
        skip = self._far_skip(ch, after)
        work_bytes = self._far_work_bytes(ch, block, views[3], abi.FH_STAKE_MAX_WORDS)
        if not 0 <= int(gain_blocks) <= abi.FH_STAKE_MAX_BLOCKS:
            raise capi.FasterHipError("Fleet.explore_far_team: gain_blocks must be 0 .. %d, got %r" % (abi.FH_STAKE_MAX_BLOCKS, gain_blocks))
        if hop_cost is not None:
            if not 0 <= int(hop_cost) <= abi.FH_STAKE_MAX_HOP_COST:
                raise capi.FasterHipError("Fleet.explore_far_team: hop_cost must be None or 0 .. %d, got %r" % (abi.FH_STAKE_MAX_HOP_COST, hop_cost))
            par["hop_cost"] = int(hop_cost)
        if int(min_gain) < 0:
            raise capi.FasterHipError("Fleet.explore_far_team: min_gain must be >= 0, got %r" % (min_gain,))
        par["min_gain"] = int(min_gain)
        if claim_blocks is not None:
            if not 0 <= int(claim_blocks) <= abi.FH_STAKE_MAX_CLAIM_BLOCKS:
                raise capi.FasterHipError("Fleet.explore_far_team: claim_blocks must be None or 0 .. %d, got %r"
                                          % (abi.FH_STAKE_MAX_CLAIM_BLOCKS, claim_blocks))
            par["claim_blocks"] = int(claim_blocks)
        return self._chooser_stages(ch, par, views, work_bytes, block, skip, groups)

    def far_team_records(self):
        """(records [n] abi.far_team_record_dtype, goals [n][3], mask [n] int32) of the last explore_far_team() (synchronises)."""
        return self._chooser_records(self.CHOOSERS["far_team"])

    def explore_spread(self, r_max, r_spread, r_avoid=None, z=None, want="reached", max_hops=0, passes=None, groups="link"):
        """explore_reachable() for a team (include/fasterhip_spread.h): a frontier voxel nearer than r_spread to the goal that a peer is
        on its way to, or that a peer with a lower index has been given by an earlier pass of this call, is not chosen, so vehicles
        with equal views that stand together fly to different places.  Peers are the vehicles of one group: groups="link" takes the
        labels of the last link() if there was one, else the view; groups="view" always the view.  passes: how long a chain of
        vehicles that wait for each other may be (None: abi.FH_SPREAD_DEFAULT_PASSES); a vehicle behind that gets no goal this period
        (FH_SPREAD_UNSETTLED) and is wanted again in the next.  The other arguments, the preconditions and the errors are those of
        explore_reachable(); the buffers and the workspace are its own (spread_records())."""
        self._run(self.explore_spread_stages(r_max, r_spread, r_avoid, z, want, max_hops, passes, groups))   # (raises before anything is launched)

    def explore_spread_stages(self, r_max, r_spread, r_avoid=None, z=None, want="reached", max_hops=0, passes=None, groups="link"):
        """The launches of explore_spread(), in order: [(name, callable)], set_goals last (scripts/fleet_cycle.py times them one by one)."""
        ch = self.CHOOSERS["spread"]
        self._check_groups(ch, groups)
        par = abi.default_spread_params(r_max, r_spread)
        views = self._chooser_inputs(ch, par, r_avoid, z, want, max_hops)   # (set_unknown's one grid: one team)
        if passes is not None:
            par["passes"] = passes
        return self._chooser_stages(ch, par, views, groups=groups)

    def spread_records(self):
        """(records [n] abi.spread_record_dtype, goals [n][3], mask [n] int32) of the last explore_spread() (synchronises)."""
        return self._chooser_records(self.CHOOSERS["spread"])

    def explore_gain(self, r_max, gain_radius, hop_cost=1, min_gain=0, r_avoid=None, z=None, want="reached", max_hops=0):
        """explore_reachable() with the choice of include/fasterhip_gain.h: of the frontier voxels that the flood reaches the one with the
        largest gain - hop_cost * hops, where the gain of a voxel is the number of unknown voxels of the view, inside the box of the
        vehicle's sphere, within gain_radius voxels of it, and the hops are the steps of the flood; among equals the fewest hops, then
        the smallest distance.  gain_radius is in voxels: sensor radius / res, rounded down, at most 31.  hop_cost: the unknown voxels
        that one step is worth (0 .. 16384); min_gain: a voxel with a smaller gain is never chosen (gain_records() counts them as poor).
        With gain_radius 0, hop_cost 1 and min_gain 0 it is explore_reachable().  The other arguments, the preconditions and the errors
        are those of explore_reachable(); the buffers are its own (gain_records())."""
        self._run(self.explore_gain_stages(r_max, gain_radius, hop_cost, min_gain, r_avoid, z, want, max_hops))   # (raises before anything is launched)

    def explore_gain_stages(self, r_max, gain_radius, hop_cost=1, min_gain=0, r_avoid=None, z=None, want="reached", max_hops=0):
        """The two launches of explore_gain(), in order: [(name, callable)] (scripts/fleet_cycle.py times them one by one)."""
        ch = self.CHOOSERS["gain"]
        par = abi.default_gain_params(r_max, gain_radius)
        par["hop_cost"], par["min_gain"] = hop_cost, min_gain
        return self._chooser_stages(ch, par, self._chooser_inputs(ch, par, r_avoid, z, want, max_hops))

    def gain_records(self):
        """(records [n] abi.gain_record_dtype, goals [n][3], mask [n] int32) of the last explore_gain() (synchronises)."""
        return self._chooser_records(self.CHOOSERS["gain"])

    def explore_sight(self, r_max, gain_radius, hop_cost=1, min_gain=0, r_avoid=None, z=None, want="reached", max_hops=0):
        """explore_gain() with a gain that the vehicle's sensor can deliver (include/fasterhip_sight.h): an unknown voxel of the ball
        counts only if the straight line of voxels from the candidate to it crosses no voxel that the view knows and the map holds
        occupied (or that lies outside the map); unknown voxels do not block.  A candidate beside a known wall is no longer promised
        the hall behind it.  gain_radius is in voxels: sensor radius / res, rounded down, at most 31.  The arguments, the preconditions
        and the errors are those of explore_gain(); the buffers are its own (sight_records()).  Where a vehicle's box holds no such
        voxel the choice is explore_gain()'s."""
        self._run(self.explore_sight_stages(r_max, gain_radius, hop_cost, min_gain, r_avoid, z, want, max_hops))   # (raises before anything is launched)

    def explore_sight_stages(self, r_max, gain_radius, hop_cost=1, min_gain=0, r_avoid=None, z=None, want="reached", max_hops=0):
        """The two launches of explore_sight(), in order: [(name, callable)] (scripts/fleet_cycle.py times them one by one)."""
        ch = self.CHOOSERS["sight"]
        par = abi.default_sight_params(r_max, gain_radius)
        par["hop_cost"], par["min_gain"] = hop_cost, min_gain
        return self._chooser_stages(ch, par, self._chooser_inputs(ch, par, r_avoid, z, want, max_hops))

    def sight_records(self):
        """(records [n] abi.sight_record_dtype, goals [n][3], mask [n] int32) of the last explore_sight() (synchronises)."""
        return self._chooser_records(self.CHOOSERS["sight"])

    def explore_team(self, r_max, r_spread, gain_radius, claim_radius=None, hop_cost=1, min_gain=0, r_avoid=None, z=None, want="reached",
                     max_hops=0, passes=None, groups="link"):
        """explore_gain() for a team (include/fasterhip_team.h): explore_gain()'s utility inside explore_spread()'s passes.  The goal
        that a peer is on its way to, or that a peer with a lower index has been given by an earlier pass, removes the candidates
        nearer than r_spread to it and, from every gain, the unknown voxels within claim_radius voxels of its voxel, which that peer's
        sensor will uncover anyway (None: gain_radius; -1: claims cover nothing; at most 31).  Two teammates before one hall get goals
        whose balls do not count the same voxels twice.  gain_radius, hop_cost and min_gain are explore_gain()'s, passes and groups
        explore_spread()'s; the other arguments, the preconditions and the errors are those of explore_reachable(); the buffers and
        the workspace are its own (team_records())."""
        self._run(self.explore_team_stages(r_max, r_spread, gain_radius, claim_radius, hop_cost, min_gain, r_avoid, z, want, max_hops, passes,
                                           groups))   # (raises before anything is launched)

    def explore_team_stages(self, r_max, r_spread, gain_radius, claim_radius=None, hop_cost=1, min_gain=0, r_avoid=None, z=None, want="reached",
                            max_hops=0, passes=None, groups="link"):
        """The launches of explore_team(), in order: [(name, callable)], set_goals last (scripts/fleet_cycle.py times them one by one)."""
        ch = self.CHOOSERS["team"]
        self._check_groups(ch, groups)
        par = abi.default_team_params(r_max, r_spread, gain_radius, claim_radius)
        par["hop_cost"], par["min_gain"] = hop_cost, min_gain
        views = self._chooser_inputs(ch, par, r_avoid, z, want, max_hops)   # (set_unknown's one grid: one team)
        if passes is not None:
            par["passes"] = passes
        return self._chooser_stages(ch, par, views, groups=groups)

    def team_records(self):
        """(records [n] abi.team_record_dtype, goals [n][3], mask [n] int32) of the last explore_team() (synchronises)."""
        return self._chooser_records(self.CHOOSERS["team"])

    def explore_bid(self, r_max, r_spread, gain_radius, claim_radius=None, hop_cost=1, min_gain=0, r_avoid=None, z=None, want="reached",
                    max_hops=0, passes=None, groups="link"):
        """explore_team() with rounds ordered by bids, not by the vehicle index (include/fasterhip_bid.h): every undecided vehicle offers
        the best candidate of explore_team()'s search under the claims so far; an offer that beats the offer of every undecided rival
        in reach (the larger utility, then the fewer hops, then the lower index) is final in that round, and the others search again
        under the new claims.  Two teammates before one hall: the one beside it gets it, whatever its index.  The arguments (claim_radius
        None: gain_radius; -1: claims cover nothing; at most 31), the preconditions and the errors are those of explore_team(); passes
        counts the rounds; the buffers and the workspace are its own (bid_records())."""
        self._run(self.explore_bid_stages(r_max, r_spread, gain_radius, claim_radius, hop_cost, min_gain, r_avoid, z, want, max_hops, passes,
                                          groups))   # (raises before anything is launched)

    def explore_bid_stages(self, r_max, r_spread, gain_radius, claim_radius=None, hop_cost=1, min_gain=0, r_avoid=None, z=None, want="reached",
                           max_hops=0, passes=None, groups="link"):
        """The launches of explore_bid(), in order: [(name, callable)], set_goals last (scripts/fleet_cycle.py times them one by one)."""
        ch = self.CHOOSERS["bid"]
        self._check_groups(ch, groups)
        par = abi.default_bid_params(r_max, r_spread, gain_radius, claim_radius)
        par["hop_cost"], par["min_gain"] = hop_cost, min_gain
        views = self._chooser_inputs(ch, par, r_avoid, z, want, max_hops)   # (set_unknown's one grid: one team)
        if passes is not None:
            par["passes"] = passes
        return self._chooser_stages(ch, par, views, groups=groups)

    def bid_records(self):
        """(records [n] abi.bid_record_dtype, goals [n][3], mask [n] int32) of the last explore_bid() (synchronises)."""
        return self._chooser_records(self.CHOOSERS["bid"])

    def coverage_stages(self):
        """The one launch of coverage(): [(name, callable)]."""
        if self.grid is None:
            raise capi.FasterHipError("Fleet.coverage: set_unknown_views (or set_unknown) first")
        flags, stride, _, n_views = self._explore_views()
        t = self.torch
        if self.d_coverage is None or self.d_coverage.numel() != n_views * abi.view_coverage_dtype.itemsize:
            self._follow_current()
            with t.cuda.stream(self.stream):
                self.d_coverage = t.zeros(n_views * abi.view_coverage_dtype.itemsize, dtype=t.uint8, device=self.dev)
            self.d_coverage.record_stream(self.stream)
        return [("view_coverage", lambda: self.map.view_coverage_device(self.grid, flags.data_ptr(), stride, n_views, self.d_coverage.data_ptr()))]

    def coverage(self):
        """[n_views] abi.view_coverage_dtype: the known voxels of every view and its frontier voxels (fh_map_view_coverage_device; one
        launch on the fleet's stream, then synchronises)."""
        stages = self.coverage_stages()
        self._follow_current()
        for _, launch in stages:
            launch()
        return self._host(self.d_coverage, abi.view_coverage_dtype)

    def point_masks(self):
        """[n_views][words] uint32 on the host (synchronises)."""
        self.sync()
        return self.point_mask.cpu().numpy().view(np.uint32).copy()

    def enable_heading(self, yaw0=None, w_max=4.0, alpha_filter_dyaw=0.0):
        """Allocates one fh_heading per vehicle (yaw = previous_yaw = yaw0[i], None: 0) and attaches the records to the context: from
        now on replan() writes look_at (M_.pos), next_goals() computes yaw and dyaw, and sense(fov=...) can look forward."""
        t = self.torch
        self.yaw_params = abi.default_yaw_params(self.dc)
        self.yaw_params["w_max"], self.yaw_params["alpha_filter_dyaw"] = w_max, alpha_filter_dyaw
        self.d_headings = t.zeros(self.n * abi.heading_dtype.itemsize, dtype=t.uint8, device=self.dev)
        self.d_goal_yaw = t.zeros((self.n, 2), dtype=t.float64, device=self.dev)
        d_yaw0 = None if yaw0 is None else self._host_to_device(np.asarray(yaw0, dtype=np.float64).reshape(self.n), t.float64)
        self._follow_current()
        with t.cuda.stream(self.stream):
            self.ctx.fleet_heading_init_device(None if d_yaw0 is None else d_yaw0.data_ptr(), self.n, self.d_headings.data_ptr())
            if d_yaw0 is not None:
                d_yaw0.record_stream(self.stream)
        self.ctx.fleet_set_headings_device(self.d_headings.data_ptr(), self.n)

    def set_goals(self, goals, mask=None):
        """setTerminalGoal for the vehicles with mask[i] != 0 (None: all): a vehicle that had reached its goal becomes YAWING."""
        t = self.torch
        d_goals = self._host_to_device(np.asarray(goals, dtype=np.float64).reshape(self.n, 3) if not isinstance(goals, t.Tensor) else goals, t.float64)
        d_mask = None
        if mask is not None:
            d_mask = self._host_to_device(np.asarray(mask).astype(np.int32).reshape(self.n) if not isinstance(mask, t.Tensor) else mask, t.int32)
        self._follow_current()
        with t.cuda.stream(self.stream):
            self.ctx.fleet_set_goals_device(self.params, self.d_vehicles.data_ptr(), d_goals.data_ptr(), None if d_mask is None else d_mask.data_ptr(),
                                            self.n)
            d_goals.record_stream(self.stream)
            if d_mask is not None:
                d_mask.record_stream(self.stream)

    def sense(self, r_sense, fov=None):
        """Every vehicle looks around from its current position and clears, in its view, the unknown flag of each voxel within r_sense
        that the occupied cells of the map do not hide (fh_fleet_sense_device: the sensor model is stated in include/fasterhip.h).  One
        launch on the fleet's stream.  fov = (tan_half_h, tan_half_v): only what lies in that field of view along the vehicle's heading
        (fh_fleet_sense_fov_device; needs enable_heading)."""
        if self.view_flags is None or self.cloud is None:
            raise capi.FasterHipError("Fleet.sense: set_map and set_unknown_views first")
        self._follow_current()
        origin, res, dims = self.grid
        if fov is not None:
            if self.d_headings is None:
                raise capi.FasterHipError("Fleet.sense: a field of view needs enable_heading first")
            self.ctx.fleet_sense_fov_device(self.map, r_sense, origin, res, dims, self.view_flags.data_ptr(), self.view_flags.shape[1],
                                            None if self.view_of is None else self.view_of.data_ptr(), self.n_views, self.d_vehicles.data_ptr(), self.n,
                                            self.d_headings.data_ptr(), fov[0], fov[1])
            return
        self.ctx.fleet_sense_device(self.map, r_sense, origin, res, dims, self.view_flags.data_ptr(), self.view_flags.shape[1],
                                    None if self.view_of is None else self.view_of.data_ptr(), self.n_views, self.d_vehicles.data_ptr(), self.n)

    def views(self):
        """[n_views][nz][ny][nx] uint8 on the host: the unknown flags of every view (synchronises)."""
        _, _, dims = self.grid
        self.sync()
        return self.view_flags.cpu().numpy().reshape(self.n_views, dims[2], dims[1], dims[0])

    # ---- one period ----
    def stages(self):
        """The launches of one replan of every vehicle, in order: [(name, callable)] (scripts/fleet_cycle.py times them one by one)."""
        if self.cloud is None or self.grid is None:
            raise capi.FasterHipError("Fleet.replan: set_map and set_unknown (or set_unknown_views) first")
        if self.round_par is None:
            return self._cycle_stages(self.d_active, self.d_check, 0)
        # priority rounds (include/fasterhip_rounds.h): begin once, into d_active_begin; the rest of the chain once per round, behind its gate
        B, c = self.n, self.ctx
        p = lambda t: t.data_ptr()  # noqa: E731
        rounds = [(r, "@%d" % r) for r in range(int(self.round_par["rounds"]))]
        rounds += [(abi.FH_ROUND_RETRY, "@retry %d" % t) for t in range(self.round_retries)]
        out = []
        for row, (rnd, tag) in enumerate(rounds):
            body = self._cycle_stages(self.d_active_begin, None if self.check_par is None else self.d_check_rounds[row], row)
            if row == 0:
                out.append(body[0])
                if not self.round_fixed:
                    out.append(("round_classes", lambda: c.fleet_round_classes_device(self.round_par, p(self.d_vehicles), p(self.d_plans), B,
                                                                                      self.max_states, self.round_cells, p(self.d_rounds))))
            out.append(("gate" + tag, lambda rnd=rnd: c.fleet_round_gate_device(p(self.d_rounds), rnd, p(self.d_active_begin), B,
                                                                                p(self.d_vehicles), p(self.d_active))))
            if self.traffic_par is not None:
                out.append(("traffic" + tag, self._traffic_launch))
            out += [(name + tag, launch) for name, launch in body[1:]]
        out.append(("gate_restore", lambda: c.fleet_round_gate_device(None, abi.FH_ROUND_RESTORE, p(self.d_active_begin), B, p(self.d_vehicles),
                                                                      p(self.d_active))))
        return out

    def _cycle_stages(self, d_active_begin, d_check, row):
        """The chain of one replan: begin writes who replans into d_active_begin (without rounds: d_active, what the path search reads),
        the check its records into d_check, a listed map_views its list into row `row` of the view lists."""
        B, P, c, m = self.n, self.params, self.ctx, self.map
        p = lambda t: t.data_ptr()  # noqa: E731
        origin, res, dims = self.grid
        # (with traffic or obstacles: the static points, the others' plans and the obstacles' points)
        n_cloud = self.n_cloud if self._tail_first() is None else self.n_cloud_all
        chain = self._shared_map_stages(B, P, c, m, p, origin, res, dims, n_cloud, d_active_begin)
        if self.check_par is not None:   # backup -> commit -> check -> revert (include/fasterhip_check.h)
            chain = chain[:-1] + [
                ("backup", lambda: c.fleet_backup_device(p(self.d_vehicles), p(self.d_plans), B, self.max_states, p(self.d_backup_vehicles),
                                                         p(self.d_backup_plans))),
                chain[-1],
                ("check", lambda: c.fleet_check_device(self.check_par, p(self.d_vehicles), p(self.d_plans), p(self.d_backup_vehicles),
                                                       p(self.d_backup_plans), B, self.max_states, self.check_cells, p(d_check))),
                ("revert", lambda: c.fleet_revert_device(p(d_check), p(self.d_backup_vehicles), p(self.d_backup_plans), B, self.max_states,
                                                         p(self.d_vehicles), p(self.d_plans))),
            ]
        if self.point_mask is None:
            return chain
        cells, mres, center, z_max, inflation = self.map_args
        vo = None if self.view_of is None else p(self.view_of)
        views = [
            ("map_views", lambda: m.read_views_device(p(self.cloud), n_cloud, p(self.point_mask), self.point_mask.shape[1], self.n_views, cells,
                                                      mres, center, self.z_ground, z_max, inflation)),
            ("path_search", lambda: m.plan_batch_radius_views_device(p(self.d_starts), p(self.d_goals), p(self.d_radius), p(self.d_active), B, self.mp,
                                                                     p(self.d_paths), p(self.d_np), vo, self.n_views, p(self.d_ex),
                                                                     self.dist_max_vertexes, 0)),
        ]
        if self.listed_views:
            lst, cnt = self.d_view_list[row], self.d_view_count[row:row + 1]
            full = views[0][1]

            def map_views():   # (full or listed is decided when the launch runs: stages() may be called any number of times before)
                if self._views_full:
                    full()
                    self._views_full = False
                else:
                    m.read_views_listed_device(p(self.cloud), n_cloud, p(self.point_mask), self.point_mask.shape[1], self.n_views, cells, mres,
                                               center, self.z_ground, z_max, inflation, p(lst), p(cnt))

            views = [("view_list", lambda: m.view_list_device(p(self.d_active), vo, B, self.n_views, p(lst), p(cnt))),
                     ("map_views", map_views), views[1]]
        return chain[:1] + views + chain[2:]

    def _shared_map_stages(self, B, P, c, m, p, origin, res, dims, n_cloud, d_active_begin):
        return [
            ("begin", lambda: c.fleet_begin_device(P, p(self.d_vehicles), p(self.d_plans), B, self.max_states, p(self.d_whole), p(self.d_safe),
                                                   p(self.d_starts), p(self.d_goals), p(self.d_radius), p(d_active_begin))),
            ("path_search", lambda: m.plan_batch_radius_device(p(self.d_starts), p(self.d_goals), p(self.d_radius), p(self.d_active), B, self.mp,
                                                               p(self.d_paths), p(self.d_np), p(self.d_ex), self.dist_max_vertexes, 0)),
            ("corridors", lambda: c.corridor_batch_device(p(self.cloud), n_cloud, p(self.d_paths), p(self.d_np), B, self.mp, self.max_poly, self.fpp,
                                                          p(self.d_wf), p(self.d_off), p(self.d_npoly), p(self.d_last), self.decomp_radius,
                                                          self.z_ground, self.local_bbox)),
            ("corridor_problems", lambda: c.corridor_problems_device(p(self.d_np), p(self.d_last), p(self.d_goals), p(self.d_wf), p(self.d_off),
                                                                     p(self.d_npoly), B, self.fpp, self.N, p(self.d_whole))),
            ("whole_solve", lambda: c.solve_batch_device(p(self.d_whole), p(self.d_wf), B, self.N, self.fpp, p(self.d_wr))),
            ("safe_corridor", lambda: c.safe_corridor_batch_device(p(self.d_whole), p(self.d_wr), p(self.d_paths), p(self.d_np), self.mp, p(self.d_goals),
                                                                   p(self.cloud), n_cloud, origin, res, dims, B, 0.5, self.max_poly,
                                                                   self.local_bbox, self.decomp_radius, self.z_ground, self.fpp, self.N,
                                                                   p(self.d_safe), p(self.d_sf), p(self.d_spaths), p(self.d_snp))),
            ("safe_solve", lambda: c.solve_batch_device(p(self.d_safe), p(self.d_sf), B, self.N, self.fpp, p(self.d_sr))),
            ("commit", lambda: c.fleet_commit_device(P, p(self.d_vehicles), p(self.d_plans), B, self.max_states, p(self.d_np), p(self.d_whole),
                                                     p(self.d_wr), p(self.d_safe), p(self.d_sr))),
        ]

    def replan(self):
        """One replan of every vehicle (asynchronous: call sync() or read an accessor to wait)."""
        self._follow_current()
        for _, launch in self.stages():
            launch()

    def next_goals(self, ticks, follow=True):
        """getNextGoal `ticks` times for every vehicle; returns the device buffer of the last goals ([n] fh_state as bytes).  follow: the
        current state becomes that goal (updateState of a vehicle that tracks its plan perfectly).  With enable_heading the yaw entry
        runs instead (1 <= ticks <= 65536): the same goals, and (yaw, dyaw) of the last one in self.d_goal_yaw ([n][2], goal_yaw())."""
        self.obstacle_tick += int(ticks)   # (the obstacle clock runs with the plans' cursor)
        self.track_tick += int(ticks)      # (and so do the clock of the sightings and the truth's)
        self.truth_tick += int(ticks)
        if self.d_headings is not None:
            self.ctx.fleet_next_goals_yaw_device(self.yaw_params, self.d_vehicles.data_ptr(), self.d_plans.data_ptr(), self.d_headings.data_ptr(),
                                                 self.n, self.max_states, int(ticks), follow, self.d_next.data_ptr(), self.d_goal_yaw.data_ptr())
            return self.d_next
        self.ctx.fleet_next_goals_device(self.d_vehicles.data_ptr(), self.d_plans.data_ptr(), self.n, self.max_states, int(ticks), follow,
                                         self.d_next.data_ptr())
        return self.d_next

    def sync(self):
        self.stream.synchronize()

    # ---- accessors (synchronise) ----
    def _host(self, t, dtype):
        self.sync()
        return t.cpu().numpy().view(dtype).copy()

    def vehicles(self):
        """[n] abi.vehicle_dtype: status, plan extent, windows, persisted safe factor and the log of the last replan."""
        return self._host(self.d_vehicles, abi.vehicle_dtype)

    def log(self):
        v = self.vehicles()
        return {k: v[k] for k in ("stage", "needed_safe", "k_end_whole", "k_safe", "index_h", "n_whole", "n_safe", "whole_factor", "safe_factor")}

    def goals(self):
        """[n] abi.state_dtype: what the last next_goals returned."""
        return self._host(self.d_next, abi.state_dtype)

    def headings(self):
        """[n] abi.heading_dtype: yaw, previous_yaw, the filtered yaw rate, the last goal's yaw and dyaw, look_at (M_) and dir."""
        if self.d_headings is None:
            raise capi.FasterHipError("Fleet.headings: enable_heading first")
        return self._host(self.d_headings, abi.heading_dtype)

    def goal_yaw(self):
        """[n][2] (yaw, dyaw) of what the last next_goals returned."""
        if self.d_goal_yaw is None:
            raise capi.FasterHipError("Fleet.goal_yaw: enable_heading first")
        self.sync()
        return self.d_goal_yaw.cpu().numpy().copy()

    def certify(self, tol=None):
        """Certificates of the last replan() (include/fasterhip_certify.h), computed on the device from the fleet's own problem, face and
        result buffers: {"whole": [n] abi.certificate_dtype, "safe": [n] abi.certificate_dtype}.  A vehicle whose stage never reached a
        solve has FH_CERT_UNSOLVED.  A measurement: nothing of the fleet changes, committing stays unconditional (synchronises)."""
        t, B = self.torch, self.n
        d_cw, d_cs = (t.zeros(B * abi.certificate_dtype.itemsize, dtype=t.uint8, device=self.dev) for _ in range(2))
        self._follow_current()
        with t.cuda.stream(self.stream):
            self.ctx.certify_batch_device(self.d_whole.data_ptr(), self.d_wf.data_ptr(), B * self.fpp, self.d_wr.data_ptr(), B, d_cw.data_ptr(), tol)
            self.ctx.certify_batch_device(self.d_safe.data_ptr(), self.d_sf.data_ptr(), B * self.fpp, self.d_sr.data_ptr(), B, d_cs.data_ptr(), tol)
            d_cw.record_stream(self.stream)
            d_cs.record_stream(self.stream)
        return {"whole": self._host(d_cw, abi.certificate_dtype), "safe": self._host(d_cs, abi.certificate_dtype)}

    def audit_device(self, r_unknown=None, r_occupied=None, cap=None, stride=1, count=0, truth=False):
        """audit() without the copy to the host: one launch on the fleet's stream; returns the device tensor of [n] fh_plan_audit records
        as bytes (asynchronous)."""
        t, B = self.torch, self.n
        radius = float(self.params["rule"]["drone_radius"])
        par = abi.default_audit_params(radius)
        if r_unknown is not None:
            par["r_unknown"] = r_unknown
        if r_occupied is not None:
            par["r_occupied"] = r_occupied
        par["cap"] = 2.0 * max(float(par["r_unknown"]), float(par["r_occupied"])) if cap is None else cap
        par["stride"], par["count"] = stride, count
        kw = {}
        if not truth:
            if self.view_flags is not None:
                kw = dict(grid=self.grid, d_flags=self.view_flags.data_ptr(), view_stride=self.view_flags.shape[1],
                          d_view_of=None if self.view_of is None else self.view_of.data_ptr(), n_views=self.n_views)
                if self.point_mask is not None:
                    kw.update(d_point_mask=self.point_mask.data_ptr(), mask_words=self.point_mask.shape[1])
            elif self.flags is not None:
                kw = dict(grid=self.grid, d_flags=self.flags.data_ptr(), view_stride=0, n_views=1)
        if self.cloud is not None and self.n_cloud > 0:
            kw.update(d_cloud=self.cloud.data_ptr(), n_cloud=self.n_cloud)
        self._follow_current()
        with t.cuda.stream(self.stream):
            d_out = t.empty(B * abi.plan_audit_dtype.itemsize, dtype=t.uint8, device=self.dev)  # (the kernel writes every byte of every record)
            self.ctx.fleet_audit_device(par, self.d_vehicles.data_ptr(), self.d_plans.data_ptr(), B, self.max_states, d_out.data_ptr(), **kw)
        return d_out

    def audit(self, r_unknown=None, r_occupied=None, cap=None, stride=1, count=0, truth=False):
        """The committed plans, the states the vehicles fly, against unknown and occupied space (include/fasterhip_audit.h): [n]
        abi.plan_audit_dtype with squared distances (abi.audit_distances takes the roots).  The radii default to
        params["rule"]["drone_radius"], cap to twice the larger of them.  Unknown space is whatever the fleet has: one grid, views, or none;
        occupied space is the cloud through the point masks of set_point_views, else the whole cloud.  truth=True passes no flags and no
        masks: the occupied side against every point.  count=params["delta_t"] audits the states the next replan cannot change.  A
        measurement: nothing of the fleet is written (synchronises)."""
        return self._host(self.audit_device(r_unknown, r_occupied, cap, stride, count, truth), abi.plan_audit_dtype)

    def separation_cells(self, cap):
        """The default grid of the separation's broad phase, (origin, res, dims): the box of set_map with res = max(cap, 1 m), coarsened
        until it has at most FH_SEP_MAX_CELLS cells.  Without a map: one cell (all pairs)."""
        if self.map_args is None:
            return ((0.0, 0.0, 0.0), 1.0, (1, 1, 1))
        cells, mres, center, z_max, _ = self.map_args
        size = [cells[a] * mres for a in range(3)]
        origin = tuple(center[a] - 0.5 * size[a] for a in range(3))
        res = max(float(cap), 1.0)
        while True:
            dims = tuple(max(1, int(np.ceil(size[a] / res))) for a in range(3))
            if dims[0] * dims[1] * dims[2] <= abi.FH_SEP_MAX_CELLS:
                return (origin, res, dims)
            res *= 2.0

    def separation_device(self, r=None, cap=None, stride=1, count=0, cells=None):
        """separation() without the copy to the host: four launches on the fleet's stream; returns the device tensor of [n]
        fh_plan_separation records as bytes (asynchronous)."""
        t, B = self.torch, self.n
        par = abi.default_separation_params(2.0 * float(self.params["rule"]["drone_radius"]) if r is None else r)
        par["cap"] = 2.0 * float(par["r"]) if cap is None else cap
        par["stride"], par["count"] = stride, count
        if cells is None:
            cells = self.separation_cells(float(par["cap"]))
        self._follow_current()
        with t.cuda.stream(self.stream):
            d_out = t.empty(B * abi.plan_separation_dtype.itemsize, dtype=t.uint8, device=self.dev)  # (the kernel writes every byte of every record)
            self.ctx.fleet_separation_device(par, self.d_vehicles.data_ptr(), self.d_plans.data_ptr(), B, self.max_states, cells, d_out.data_ptr())
        return d_out

    def separation(self, r=None, cap=None, stride=1, count=0, cells=None):
        """The committed plans against each other, instant by instant (include/fasterhip_separation.h): [n] abi.plan_separation_dtype with
        squared distances (abi.separation_distances takes the roots).  r defaults to 2 params["rule"]["drone_radius"], where two hulls
        touch, cap to 2 r.  cells = (origin, res, dims) is the grid of the broad phase, by default separation_cells(cap); no field of a
        record depends on it.  Record i tests the instants of plan i only: the closest approach of a pair is the smaller of its two
        records' values.  count=params["delta_t"] looks at the states the next replan cannot change.  A measurement: nothing of the
        fleet is written; vehicles still do not avoid each other unless enable_traffic (synchronises)."""
        return self._host(self.separation_device(r, cap, stride, count, cells), abi.plan_separation_dtype)

    def faces(self):
        """The face rows of the last cycle on the host: {"whole": [n * faces_per_problem] abi.face_dtype, "safe": the same}; the problems
        of results() address them through face_begin / face_off (diagnostics)."""
        return {"whole": self._host(self.d_wf, abi.face_dtype), "safe": self._host(self.d_sf, abi.face_dtype)}

    def plans(self):
        """[n] lists of committed states (abi.state_dtype arrays), front first."""
        v = self.vehicles()
        raw = self._host(self.d_plans, abi.state_dtype).reshape(self.n, self.max_states)
        return [raw[i, v["plan_head"][i]:v["plan_head"][i] + v["plan_size"][i]].copy() for i in range(self.n)]

    def results(self):
        """The whole and safe problems and results of the last cycle (diagnostics)."""
        return {"whole": self._host(self.d_whole, abi.problem_dtype), "safe": self._host(self.d_safe, abi.problem_dtype),
                "wres": self._host(self.d_wr, abi.result_dtype), "sres": self._host(self.d_sr, abi.result_dtype),
                "n_points": self.d_np.cpu().numpy(), "paths": self.d_paths.cpu().numpy()}
