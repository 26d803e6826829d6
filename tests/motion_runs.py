"""The slab runs with wall motion, the inlet profile and the module clamps: which case runs in how
many ranks, along which axis, with which cuts and checkpoints (tests/test_gpu_dist_motion.py), and
what each run is taken to reach (tests/test_slab_motion_model.py proves that on the oracle alone).

Cuts.  Walls sit on a lattice of dx and move a few hundredths of dx in the checked steps (the
rigid walls 0.02 m/s x 1e-4 s per step plus the rotation, the rolling tank ~0.13 dx in 100 steps at
0.1 m from its centre, ~0.016 dx in the 3-D box), so a cut lies that close beside a wall column, on
the side the column moves to.  The halo is 2.6 dx: the band limits of a cut c are c +- 2.6 dx,
0.4 / 0.6 dx from the nearest columns when c is beside one.  No wall here moves 0.4 dx in 100
steps, so ONE cut cannot have walls cross it and its band limits both: a run in 2 ranks reaches
either owner changes or band changes, a run in 3 ranks takes one cut for each.
"""
from dataclasses import dataclass

import numpy as np

from particlemethod_fsi_amd import cases, solver

import dist_worker


@dataclass(frozen=True)
class Run:
    case: str                 # dist_worker.case_axis form: "name" or "name@axis"
    world: int
    local: bool               # slab-local creation
    cuts: tuple | None        # explicit cuts (dist_worker.make_cuts), None: equal slabs
    checkpoints: tuple
    wall_owner_changes: int = 0   # at least this many wall particles change owner (first -> last checkpoint)
    wall_band_changes: int = 0    # ... change band class and keep their owner
    seam_crossing: bool = False   # a fluid particle goes from the last rank to rank 0
    structure: bool = False       # compared with STRUCT_FIELDS / elastic_rel
    env: tuple = ()               # environment of the ranks, ((name, value), ...)

    @property
    def id(self):
        return "%s-w%d%s" % (self.case, self.world, "-local" if self.local else "")

    @property
    def name(self):
        return dist_worker.case_axis(self.case)[0]

    @property
    def axis(self):
        return dist_worker.case_axis(self.case)[1]


_FORCED = (("MPH_SLAB_OVERLAP", "1"), ("MPH_SLAB_EARLY", "1"))   # the "on" half of the bitwise pairs
_OVERLAP = (("MPH_SLAB_OVERLAP", "1"),)
# movwall2d_slab: Time 0.197 + k 1e-4 -- the walls move in steps 1..30; 25 -> 34 is a batch across 0.2
_MW = (1, 25, 34, 40)

RUNS = (
    # left wall (type 4) columns cross the cut
    Run("movwall2d_slab", 2, False, (-0.00048,), _MW, wall_owner_changes=4),
    # right wall (type 5) crosses the second cut, the left wall the first cut's lower band limit
    Run("movwall2d_slab", 3, True, (0.00212, 0.20047), _MW, wall_owner_changes=4, wall_band_changes=4, env=_FORCED),
    Run("movwall3d_slab", 2, False, (0.02551,), _MW, wall_owner_changes=4),
    Run("movwall3d_slab@2", 2, False, (0.01187,), _MW, wall_band_changes=4),
    Run("rolling2d", 3, True, (-0.00047, 0.19793), (1, 50, 100), wall_owner_changes=4, wall_band_changes=4,
        env=_FORCED),
    Run("rolling3d", 2, False, (0.025505,), (1, 50, 100), wall_owner_changes=4, env=_OVERLAP),
    Run("turek2d", 3, True, (0.22, 0.9), (1, 10, 100), seam_crossing=True, structure=True, env=_FORCED),
    Run("turek2d_fluid", 4, True, None, (1, 10, 100), seam_crossing=True, env=_FORCED),
    Run("turek2d_t07", 2, False, None, (1, 10), structure=True),
    Run("hydro2d", 3, False, None, (1, 10, 30), structure=True, env=_OVERLAP),
    Run("hydro2d", 3, True, None, (1, 10, 30), structure=True),
    Run("gate2d_rolling1", 2, True, (0.1025,), (1, 10, 30), structure=True),
)
BY_ID = {r.id: r for r in RUNS}


def build(run):
    return cases.get(run.name).build()


def owners(cfg, run, coords):
    """The owner rank of each slab coordinate (mph_slab_owner, as a slab context decides it)."""
    return np.array([solver.slab_owner(cfg, run.world, run.axis, float(a), run.cuts) for a in coords], np.int32)


def in_band(cfg, run, coords, owner):
    """Whether each coordinate lies in one of its owner's two bands (the rule of slab_class: within
    the halo of the lower face, or within or on it at the upper face)."""
    out = np.zeros(len(coords), bool)
    for r in range(run.world):
        lo, hi, h = solver.slab_bounds(cfg, r, run.world, run.axis, run.cuts)
        m = owner == r
        out[m] = ((coords[m] - lo) < h) | ((hi - coords[m]) <= h)
    return out


def static_owners(cfg, run, parts, position):
    """Owners as the slab layer assigns them: structure particles by InitialPosition (static), all
    others by `position`."""
    struct = (parts.property == 2) | (parts.property == 3)
    a = np.where(struct, parts.initial_position[:, run.axis], position[:, run.axis])
    return owners(cfg, run, a)
