/*
 * mph_gpu.h -- C ABI of the MI355X-native MPH explicit hot path (libmph_gpu.so).
 *
 * Drop-in boundary for the reference solver Ryo1011gd/ParticleMethod_FSI (src/main.cpp).
 * The reference has no plugin/FFI layer: its hot path is a set of `static void calculateX(void)`
 * functions over file-scope globals (main.cpp:200-241) called in a fixed order by main()
 * (main.cpp:581-688).  This header replaces that whole layer with a context object:
 *
 *   reference                                              | this ABI
 *   -------------------------------------------------------+--------------------------------------
 *   readDataFile          main.cpp:729-786                 | mph_read_data_file
 *   readGridFile          main.cpp:788-955                 | mph_read_grid_header/_particles
 *   initializeWeight/Fluid/Wall/Domain main.cpp:534-537,    | mph_create  (derives every constant,
 *     1191-1469; acc update device main.cpp:549-560;       |   uploads, builds the structure
 *     calculateInitialNeighbor/Neighbor/DensityA/          |   Lagrangian lists and normalizer,
 *     GravityCenter/DensityP/Lamesconstant/Normalizer      |   runs the init sums)
 *     main.cpp:564-570                                     |
 *   one iteration of the time loop main.cpp:597-686       | mph_step(ctx, 1)
 *   acc update host main.cpp:987-989 + array reads         | mph_get
 *   writeProfFile main.cpp:957-982                         | mph_write_prof
 *   writeVtkFile  main.cpp:984-1189                        | mph_write_vtk
 *   err_malloc/err_fopen exit(1) errorfunc.cpp:8-31        | negative MphStatus + mph_last_error
 *
 * Data at the boundary is the reference's own layout (vec3T.hpp:31-34 / main.cpp:105-197):
 * AoS double[n][3] for vectors, row-major double[n][3][3] for tensors, int[n] for ints, always in
 * the ORIGINAL particle order of the .grid file.  Internally the device keeps a cell-sorted
 * struct-of-arrays copy and a permutation; nothing of that leaks through this header.
 *
 * Threading: one host thread per context; several contexts may coexist (no global state).
 * mph_step is stream-ordered; mph_get/mph_write_* synchronise.
 */
#ifndef MPH_GPU_H_INCLUDED
#define MPH_GPU_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPH_TYPE_COUNT 6            /* main.cpp:68 */
#define MPH_MAX_NEIGHBOR_COUNT 512  /* main.cpp:100 (semantic limit; overflow is an error here) */
/* Bumped on every incompatible change of a declaration below (3: mph_slab_bounds/_owner/_window
 * take `cuts`; mph_dist_info slot 0/2 meaning; 5: mph_list_layout added; 6: the monitors); bindings
 * compare mph_abi_version() with it.                                                          */
#define MPH_ABI_VERSION 6

/* Compile-time case modules of the reference (main.cpp:54-59) as a runtime switch.  The module
 * selects the clamp rule of updateElasticPosition (main.cpp:1918-2044).                        */
typedef enum MphModule {
    MPH_MODULE_BAR = 0,          /* Bar_Module: x0.x < 0.001 clamped, force zeroed   (1918-1943) */
    MPH_MODULE_DAM = 1,          /* DAM_Module: x0.y < 0.002 clamped, force zeroed   (1967-1992) */
    MPH_MODULE_TUREK_HRON = 2,   /* Turek_Hron: x0.x < 0.205 clamped                 (1944-1966) */
    MPH_MODULE_ROLLING1 = 3,     /* Rolling1:   x0.y < 0.003 clamped, force zeroed   (1993-2018) */
    MPH_MODULE_HYDROELASTIC = 4, /* Hydroelastic: x0.x<0.01||>1.99, force zeroed     (2019-2044) */
    MPH_MODULE_NONE = 5          /* no clamp (only the unconditional drift of 2070-2079)          */
} MphModule;

/* calculateWall (main.cpp:2963-3072): the shipped rigid motion (the `#else` branch 3031-3071:
 * rotation WallRotation + translation WallVelocity while Time < 0.2) or the compile-time
 * `Rolling` branch (2974-3030: every step the walls turn about z through WallCenter by
 * dtheta = MAX_ANGLE [sin(w t) - sin(w (t - Dt))], w = 2 pi / ROLLING_PERIOD, main.cpp:2959-2960). */
typedef enum MphWallMotion {
    MPH_WALL_RIGID = 0,
    MPH_WALL_ROLLING = 1
} MphWallMotion;

typedef enum MphStatus {
    MPH_OK = 0,
    MPH_ERR_ARG = -1,
    MPH_ERR_IO = -2,
    MPH_ERR_NEIGHBOR_OVERFLOW = -3,  /* a particle found >= 512 neighbours (main.cpp:1766-1768) */
    MPH_ERR_DEVICE_OOM = -4,
    MPH_ERR_HIP = -5,
    MPH_ERR_RCCL = -6,
    MPH_ERR_DOMAIN = -7,             /* domain too small for the cell stencil        */
    MPH_ERR_UNSUPPORTED = -8,
    MPH_ERR_NONFINITE = -9,
    MPH_ERR_TRANSPORT = -10,         /* slab mode: host exchange callback failed                  */
    MPH_ERR_CAPACITY = -11           /* slab mode: local arrays full, or a particle jumped a slab */
} MphStatus;

/* Everything the reference reads from its .data file (main.cpp:743-767) and .grid header
 * (main.cpp:797-804), plus the two compile-time switches.  All derived constants (radii, kernel
 * normalisations, N0a/N0p, CofA, cell grid, wall rotations ...) are computed inside mph_create
 * exactly as initializeWeight/Fluid/Wall/Domain do.                                             */
typedef struct MphConfig {
    int    dim;                       /* 2 or 3: TWO_DIMENSIONAL main.cpp:50 */
    int    module;                    /* MphModule */
    double dt;                        /* Dt */
    double elastic_dt;                /* ElasticDt */
    double output_interval;           /* OutputInterval */
    double vtk_output_interval;       /* VtkOutputInterval */
    double end_time;                  /* EndTime */
    double radius_ratio_a;            /* RadiusRatioA (RadiusRatioG = RadiusRatioA, main.cpp:1193) */
    double radius_ratio_p;            /* RadiusRatioP */
    double radius_ratio_v;            /* RadiusRatioV */
    double density[MPH_TYPE_COUNT];
    double bulk_modulus[MPH_TYPE_COUNT];
    double bulk_viscosity[MPH_TYPE_COUNT];
    double shear_viscosity[MPH_TYPE_COUNT];
    double surface_tension[MPH_TYPE_COUNT];   /* .data gives types 0,1,4,5 (main.cpp:756) */
    double young_modulus[MPH_TYPE_COUNT];     /* .data gives types 2..5     (main.cpp:757) */
    double poisson_ratio[MPH_TYPE_COUNT];     /* .data gives types 2..5     (main.cpp:758) */
    double interaction_ratio[MPH_TYPE_COUNT][MPH_TYPE_COUNT];
    double gravity[3];
    double wall_center[MPH_TYPE_COUNT][3];    /* only Wall6/Wall7 -> types 4/5 are parsed (766-767) */
    double wall_velocity[MPH_TYPE_COUNT][3];
    double wall_omega[MPH_TYPE_COUNT][3];
    double time;                      /* .grid line 1 (restart time) */
    double particle_spacing;          /* .grid line 2 */
    double domain_min[3];
    double domain_max[3];
    int    wall_motion;               /* MphWallMotion (compile-time `Rolling`, main.cpp:58) */
} MphConfig;

/* sizeof(MphConfig) as compiled into the library (FFI bindings check their mirror against it). */
int mph_config_sizeof(void);
/* MPH_ABI_VERSION as compiled into the library.                                              */
int mph_abi_version(void);

/* Per-particle arrays readable with mph_get (original particle order). */
typedef enum MphField {
    MPH_FIELD_POSITION = 0,           /* double[n][3] */
    MPH_FIELD_INITIAL_POSITION = 1,   /* double[n][3] */
    MPH_FIELD_VELOCITY = 2,           /* double[n][3] */
    MPH_FIELD_FORCE = 3,              /* double[n][3] */
    MPH_FIELD_ACCELERATION = 4,       /* double[n][3] */
    MPH_FIELD_GRAVITY_CENTER = 5,     /* double[n][3] */
    MPH_FIELD_PRESSURE_P = 6,         /* double[n] */
    MPH_FIELD_PRESSURE_A = 7,         /* double[n] */
    MPH_FIELD_DENSITY_A = 8,          /* double[n] */
    MPH_FIELD_VOL_STRAIN_P = 9,       /* double[n] */
    MPH_FIELD_DIVERGENCE_P = 10,      /* double[n] */
    MPH_FIELD_MASS = 11,              /* double[n] */
    MPH_FIELD_KAPPA = 12,             /* double[n] */
    MPH_FIELD_LAMBDA = 13,            /* double[n] */
    MPH_FIELD_MU = 14,                /* double[n] */
    MPH_FIELD_NEIGHBOR_COUNT = 15,    /* int[n] */
    MPH_FIELD_INITIAL_STRUCTURE_NEIGHBOR_COUNT = 16, /* int[n] */
    MPH_FIELD_PROPERTY = 17,          /* int[n] */
    MPH_FIELD_DEFORM_GRADIENT = 18,   /* double[n][3][3] */
    MPH_FIELD_STRAIN = 19,            /* double[n][3][3] */
    MPH_FIELD_STRESS = 20,            /* double[n][3][3] */
    MPH_FIELD_NORMALIZER = 21,        /* double[n][3][3] */
    MPH_FIELD_LAMBDA_LAMES = 22,      /* double[n] */
    MPH_FIELD_MU_LAMES = 23,          /* double[n] */
    MPH_FIELD_VIRIAL_STRESS = 24,     /* double[n][3][3], VirialStressAtParticle (mph_compute_virial) */
    MPH_FIELD_VIRIAL_PRESSURE = 25,   /* double[n], VirialPressureAtParticle (mph_compute_virial) */
    MPH_FIELD_COUNT = 26
} MphField;

typedef struct MphCtx MphCtx;

/* ---- host-side file formats (no device needed) ------------------------------------------- */

/* Fill cfg with the reference's static defaults (zeros, Dt=ElasticDt=1e100) for dim/module. */
int mph_config_default(MphConfig* cfg, int dim, int module);
/* .data keyword file, main.cpp:729-786.  Unknown lines are ignored like the reference.      */
int mph_read_data_file(const char* path, MphConfig* cfg);
/* .grid / .prof header (Time; N dx xmin xmax ymin ymax zmin zmax), main.cpp:796-804.
 * Both readers also accept the binary grid of mph_write_grid_binary (detected by its magic).  */
int mph_read_grid_header(const char* path, MphConfig* cfg, int* n);
/* .grid / .prof body: n lines "type x y z x0 y0 z0 vx vy vz", main.cpp:896-904.             */
int mph_read_grid_particles(const char* path, int n, int* property, double* pos, double* pos0,
                            double* vel);
/* Binary grid (the input-path variant of SURVEY 8f: the ASCII .grid of a 16M-particle case is
 * 2 GB and takes the generator 33 s): magic "MPHGRIDB", int32 version 1, int32 n, double time,
 * dx, domain_min[3], domain_max[3], then int32 property[n] (zero-padded to 8 bytes) and
 * double position[n][3], initial_position[n][3], velocity[n][3], little endian.  The values
 * are stored exactly (no %e rounding).                                                        */
int mph_write_grid_binary(const char* path, const MphConfig* cfg, int n, const int* property,
                          const double* pos, const double* pos0, const double* vel);
/* .prof writer with the reference's exact format, main.cpp:957-982.                          */
int mph_write_prof_arrays(const char* path, const MphConfig* cfg, double time, int n,
                          const int* property, const double* pos, const double* pos0,
                          const double* vel);
/* legacy-ASCII .vtk writer with the reference's exact format, main.cpp:984-1189.            */
int mph_write_vtk_arrays(const char* path, int n, const int* property, const double* pos,
                         const double* pos0, const double* vel, const double* accel,
                         const double* force, const double* stress, const double* strain,
                         const int* initial_structure_neighbor_count, const int* neighbor_count);

/* Binary VTK XML (.vtu) alternative to the ASCII writer: the same point fields as
 * mph_write_vtk_arrays, Float32/Int32 in raw appended data (UInt64 headers), stress and strain as
 * 9-component tensors, one VTK_VERTEX cell per particle.                                       */
int mph_write_vtu_arrays(const char* path, int n, const int* property, const double* pos,
                         const double* pos0, const double* vel, const double* accel,
                         const double* force, const double* stress, const double* strain,
                         const int* initial_structure_neighbor_count, const int* neighbor_count);

/* setInitialVelocityProfile (main.cpp:395-441) on host arrays (original order; vel is updated in
 * place).  Bar_Module: the beam's first bending mode on the structure particles, v = (0,
 * 0.01 c0 f(x0)/f(L), 0) with c0 = sqrt(3.25e6/Density) and f of main.cpp:387-392 (the
 * reference's only call, main.cpp:571, is commented out: an explicit option).  Turek_Hron: the
 * parabolic inlet on fluid particles with x <= 0.01 and, while time < 0.7, x > 1.5 -- the
 * reference calls it every step before calculateWall (main.cpp:592-594), which mph_step does on
 * the device by itself for MPH_MODULE_TUREK_HRON.  Other modules: no change.                   */
int mph_velocity_profile_arrays(const MphConfig* cfg, double time, int n, const int* property,
                                const double* pos, const double* pos0, double* vel);

/* Every constant the reference derives before its time loop (initializeWeight/Fluid/Wall/Domain,
 * main.cpp:1191-1469), without a device: 36 doubles in the slot order of mph_get_scalars.      */
int mph_derive_scalars(const MphConfig* cfg, double* out36);
/* Host-side initialisation of the elastic solid that mph_create performs: the fixed Lagrangian
 * neighbour lists (calculateInitialNeighbor, main.cpp:1497-1658), calculateLamesconstant
 * (2526-2540) and calculateNormalizer (2544-2653).  Outputs are per particle, original order,
 * zero for non-structure particles: isnc int[n], normalizer double[n][3][3], lame_l/lame_m
 * double[n].  Any output pointer may be NULL.                                                   */
int mph_structure_init(const MphConfig* cfg, int n, const int* property, const double* pos0,
                       int* isnc, double* normalizer, double* lame_l, double* lame_m);

/* ---- device context ------------------------------------------------------------------------ */

/* Create a context on HIP device `device`, upload the particles, derive all constants and run
 * the reference's initialisation sums (main.cpp:534-570).                                    */
int mph_create(MphCtx** ctx, const MphConfig* cfg, int n, const int* property,
               const double* pos, const double* pos0, const double* vel, int device);
/* Advance nsteps time steps (main.cpp:597-686 each).  Steps are replayed from captured
 * hipGraphs of 8 and 1 steps; returns MPH_ERR_NEIGHBOR_OVERFLOW if any particle reached 512
 * neighbours.  The output-only fields (Force, Acceleration, DensityA, VolStrainP, DivergenceP,
 * and GravityCenter/PressureA without surface tension) are stored by the call's last step (and by
 * the last step of its last whole batch of 8), so after a successful mph_step they hold that
 * step's values; after an error
 * they are undefined (the state itself -- Position, Velocity -- is the failing step's).
 * The overflow is reported when the call returns.  A lean step (mph_lean_step_stats) counts
 * only the pairs within the list radius (MaxRadius), so a count that passes 512 only through pairs
 * of the shell MaxRadius < r <= MaxRadius + MARGIN raises the error at the next step that counts
 * every pair -- the last step of the call's last whole batch, or the call's last step: later in the
 * call by up to its length, and still in the mph_step call that took the step.                 */
int mph_step(MphCtx* ctx, int nsteps);
/* Step batching for the drop-in loop that calls mph_step(ctx, 1) once per iteration
 * (INTEGRATION.md section 2); single contexts only (slab mode: MPH_ERR_ARG for on != 0).
 * With it on, mph_step only counts the steps and launches them 8 at a time from the 8-step
 * graph, with the output-only stores on each batch's last step -- the cost of one
 * mph_step(ctx, 8) instead of eight synchronised single steps.  Time (mph_time) advances per call.
 * Steps still pending run, and the error flags of everything launched are read, at the next
 * flush point: mph_synchronize, mph_get, mph_set, every writer, mph_compute_virial,
 * mph_neighbor_stats, mph_profile_steps, mph_phase_timing, mph_monitor_configure, mph_monitor_read,
 * mph_sample_grid, mph_gauge_configure, mph_gauge_grid, mph_select and the selection's consumers,
 * mph_compute_kinematics (and _timed), mph_get_kinematics (and _selected), mph_write_vtu_kinematics
 * (and _selected), turning batching off, mph_destroy; so
 * every field read after a step is that step's, bit for bit as without batching.  A launched
 * batch's error is also reported by a later mph_step once its flags have landed (no wait).
 * Errors therefore surface up to two batches late, or at the next flush point.  Off by default. */
int mph_set_step_batching(MphCtx* ctx, int on);
/* Wait for all work the context enqueued (slab mode: both of its streams); with step batching,
 * launches the pending steps first and returns their status. */
int mph_synchronize(MphCtx* ctx);
/* Copy a field to host, AoS, original particle order.                                      */
int mph_get(MphCtx* ctx, int field, void* host_out);
/* Overwrite Position or Velocity (original order) -- the reference's `acc update device`.    */
int mph_set(MphCtx* ctx, int field, const void* host_in);
/* setInitialVelocityProfile() (main.cpp:395-441) applied once to the current state, as the
 * reference's commented call after the initialisation sums would (main.cpp:571); see
 * mph_velocity_profile_arrays.                                                                */
int mph_set_initial_velocity_profile(MphCtx* ctx);
int mph_particle_count(const MphCtx* ctx);
double mph_time(const MphCtx* ctx);
/* Derived scalar constants, same slots as oracle/ref_harness.inc ref_scalars (36 doubles).  */
int mph_get_scalars(const MphCtx* ctx, double* out36);
/* The output files of the whole problem.  Slab mode: collective calls (every rank at the same
 * step); each rank's owned particles are gathered on rank 0 (RCCL: one receive per rank; host
 * transport: along the ring of neighbour exchanges), which writes `path` -- the same bytes as a
 * single context holding the same state; the other ranks write nothing.                        */
int mph_write_prof(MphCtx* ctx, const char* path);
int mph_write_vtk(MphCtx* ctx, const char* path);
int mph_write_vtu(MphCtx* ctx, const char* path);   /* mph_write_vtu_arrays of the current state */
/* writeVtkFile (main.cpp:984-1189) off the time loop's critical path: the fields are copied to
 * host memory now (one D2H per field) and formatted and written by a background thread while
 * the following steps run.  At most one file is in flight; mph_output_wait joins it and
 * returns its status (also called by the next mph_write_vtk_async and by mph_destroy).
 * The bytes are those of mph_write_vtk.                                                        */
int mph_write_vtk_async(MphCtx* ctx, const char* path);
int mph_output_wait(MphCtx* ctx);
/* Message of the last failure on ctx; with ctx == NULL, of the last failed mph_create* on the
 * calling thread (the context is destroyed on failure).                                        */
const char* mph_last_error(const MphCtx* ctx);
void mph_destroy(MphCtx* ctx);

/* calculateVirialStressAtParticle (main.cpp:3077-3318), which the reference runs after the
 * physics of every VTK output step (main.cpp:672-673): per-particle virial stress of the
 * pressure (PressureP, PressureA), viscous and diffuse-interface pair forces over the step's
 * neighbour list at the post-step positions and velocities, and VirialPressureAtParticle
 * = -tr/dim.  Results are read with mph_get(MPH_FIELD_VIRIAL_STRESS / _PRESSURE); zeros until
 * the first call.  Slab mode: collective; every rank computes its owned particles, after one halo
 * exchange of the ghosts' post-step positions and velocities.                               */
int mph_compute_virial(MphCtx* ctx);

/* ---- per-step monitors ------------------------------------------------------------------------ */

/* A time history without mph_get: while monitors are on, every step (whichever way mph_step runs
 * it: the captured graphs, step batching, phase timing, mph_profile_steps) ends with kernels that
 * reduce the state the step leaves into one record, the sample, and every `stride`-th step's
 * sample is kept in a ring buffer on the device.  Reading the ring is a flush point like mph_get,
 * stepping is not.  With monitors off a step is what it was.  Single contexts only.
 *
 * A sample is MPH_MONITOR_HEAD doubles (MphMonitorSlot), then {x, y, z, vx, vy, vz} per tracked
 * particle, then {value, count} per probe.  Every slot but the probes is the named function of
 * what mph_get would return for Position, Velocity, PressureP and Property right after that step;
 * the mass of a particle is Density[type] * V (MPH_FIELD_MASS).  Sums are taken in an order fixed
 * by the particle count, so the same state gives the same bits in any batch shape.  Extrema over
 * no particle: +inf for a minimum, -inf for a maximum, 0 for VMAX2.
 * Probe q: the Shepard average of the step's PressureP over the fluid particles within
 * probe_radius h of the probe, value = sum w P / sum w with w = (1 - r/h)^2 for r < h, r the
 * minimum-image distance to the position PressureP was computed at (the step's sorted set: the
 * wrapped position before the step's motion); count = the contributing particles; no particle in
 * range: value = count = 0.  2-D: a probe's z is ignored.                                        */
#define MPH_MONITOR_MAX_TRACK  64
#define MPH_MONITOR_MAX_PROBES 64
#define MPH_MONITOR_HEAD       32
typedef enum MphMonitorSlot {
    MPH_MON_STEP = 0,            /* steps since mph_monitor_configure at which the sample was taken */
    MPH_MON_TIME = 1,            /* == mph_time after that step, bit for bit                        */
    /* per class, six slots: COUNT, KE = sum 1/2 m v.v, PX PY PZ = sum m v, VMAX2 = max v.v
     * (vx vx + vy vy + vz vz left to right, no contraction)                                       */
    MPH_MON_FLUID_COUNT = 2,     /* fluid: types 0, 1 */
    MPH_MON_FLUID_KE = 3,
    MPH_MON_FLUID_PX = 4,
    MPH_MON_FLUID_PY = 5,
    MPH_MON_FLUID_PZ = 6,
    MPH_MON_FLUID_VMAX2 = 7,
    MPH_MON_STRUCT_COUNT = 8,    /* structure: types 2, 3 */
    MPH_MON_STRUCT_KE = 9,
    MPH_MON_STRUCT_PX = 10,
    MPH_MON_STRUCT_PY = 11,
    MPH_MON_STRUCT_PZ = 12,
    MPH_MON_STRUCT_VMAX2 = 13,
    MPH_MON_WALL_COUNT = 14,     /* walls: types 4, 5 */
    MPH_MON_WALL_KE = 15,
    MPH_MON_WALL_PX = 16,
    MPH_MON_WALL_PY = 17,
    MPH_MON_WALL_PZ = 18,
    MPH_MON_WALL_VMAX2 = 19,
    MPH_MON_XMIN = 20,           /* bounding box of the fluid */
    MPH_MON_XMAX = 21,
    MPH_MON_YMIN = 22,
    MPH_MON_YMAX = 23,
    MPH_MON_ZMIN = 24,
    MPH_MON_ZMAX = 25,
    MPH_MON_FLUID_PMIN = 26,     /* PressureP over the fluid */
    MPH_MON_FLUID_PMAX = 27,
    MPH_MON_WALL_PMAX = 28,      /* PressureP over the walls */
    MPH_MON_EPOT = 29,           /* - sum m (g . x) over fluid and structure particles */
    MPH_MON_RESERVED0 = 30,      /* zero */
    MPH_MON_RESERVED1 = 31
} MphMonitorSlot;
typedef struct MphMonitorConfig {
    int stride;            /* sample the steps k = stride, 2 stride, ... counted from this call (>= 1) */
    int capacity;          /* samples the device ring holds (>= 1) */
    int ntrack;            /* tracked particles (original indices), 0..MAX_TRACK */
    const int* track;
    int nprobe;            /* pressure probes, 0..MAX_PROBES */
    const double* probes;  /* [nprobe][3], wrapped into the periodic domain like a particle */
    double probe_radius;   /* 0: RadiusRatioP * dx; must be <= MaxRadius + MARGIN (the cell stencil's reach) */
} MphMonitorConfig;
/* Turn monitors on with *cfg (replacing an earlier configuration: the ring is emptied, STEP counts
 * from this call) or, cfg == NULL, off.  A flush point; the step graphs are captured again at the
 * next step.  MPH_ERR_ARG: stride or capacity < 1, a count over its maximum, a track index outside
 * [0, n), a probe radius below 0 or over the stencil's reach.  MPH_ERR_UNSUPPORTED: slab mode.   */
int mph_monitor_configure(MphCtx* ctx, const MphMonitorConfig* cfg);
/* Doubles per sample: MPH_MONITOR_HEAD + 6 ntrack + 2 nprobe (+ MPH_GAUGE_CHANNELS ngauge after
 * mph_gauge_configure); 0 with monitors off.                                                    */
int mph_monitor_sample_doubles(const MphCtx* ctx);
/* Copy the unread samples, oldest first and at most max_samples, to out ([k][sample doubles]) and
 * return how many.  The ring keeps the newest `capacity` samples: *lost (may be NULL) receives how
 * many unread samples were overwritten since the last read.  A flush point, like mph_get.        */
long long mph_monitor_read(MphCtx* ctx, double* out, long long max_samples, long long* lost);

/* ---- per-step monitors on slab ranks ------------------------------------------------------------ */

/* The monitors of a slab context (mph_create_slab and its kin).  The calls above keep refusing one:
 * what a rank records is a partial sample, and reading a whole one is a collective call.  With slab
 * monitors on, every slab step ends with the same kernels over the rank's particles and leaves, on a
 * sampled step, one rank record of MPH_MONITOR_HEAD + 7 ntrack + 2 nprobe doubles in the rank's ring:
 *   head      MphMonitorSlot over the particles the rank owns at that step (what mph_get returns from
 *             it), each through the arithmetic of a single context; STEP and TIME as there;
 *   tracked k {present, x, y, z, vx, vy, vz}: present = 1 and the row on the rank that owns the
 *             particle at that step, seven zeros on every other rank (indices are original ones of
 *             the whole problem, [0, n) of mph_particle_count);
 *   probe q   {value, count} on the rank whose slab holds the probe's coordinate along the slab axis
 *             (wrapped like a particle's; mph_slab_owner with the context's cuts), which evaluates it
 *             over its owned particles and its ghosts; {0, -1} on every other rank.
 * No exchange is added to a step and no rank waits for another.                                    */
/* mph_monitor_configure for a slab context; every rank passes the same configuration (cfg == NULL:
 * off).  The same argument rules.  MPH_ERR_UNSUPPORTED on a single context (mph_monitor_configure). */
int mph_dist_monitor_configure(MphCtx* ctx, const MphMonitorConfig* cfg);
/* Doubles per rank record; 0 with slab monitors off.                                               */
int mph_dist_monitor_record_doubles(const MphCtx* ctx);
/* This rank's unread rank records, oldest first: mph_monitor_read's ring and *lost, no communication. */
long long mph_dist_monitor_read_partial(MphCtx* ctx, double* out, long long max_samples, long long* lost);
/* The ranks' records made samples: records[r] is rank r's [nsamples][32 + 7 ntrack + 2 nprobe], out
 * receives [nsamples][32 + 6 ntrack + 2 nprobe], the layout of mph_monitor_read.  Host only, no
 * context.  Every head slot combines by its kind -- sum, minimum, maximum -- from rank 0's value
 * through ranks 1, 2, ... in order, in plain FP64 (EPOT: the ranks' own negated sums); STEP must be the
 * same on every rank, TIME is rank 0's; a tracked entry is the row of the one rank with present == 1, a
 * probe the pair of the one rank with count >= 0.  The result is a function of the records and of the
 * rank order, bit for bit.  MPH_ERR_ARG: unequal STEP, an entry or a probe on no rank or on several. */
int mph_monitor_combine(int nranks, int ntrack, int nprobe, long long nsamples, const double* const* records,
                        double* out);
/* Collective (every rank, with the same max_samples): each rank reads its unread records, rank 0
 * gathers and combines them and returns the number of samples in out; every other rank returns 0 and
 * may pass out == NULL only with max_samples == 0.  *lost is the rank's own.  MPH_ERR_TRANSPORT on
 * rank 0: the ranks' unread counts differ.                                                          */
long long mph_dist_monitor_read(MphCtx* ctx, double* out, long long max_samples, long long* lost);

/* ---- lattice sampling ------------------------------------------------------------------------- */

/* Fields on a regular lattice without mph_get: the monitors' probe, evaluated on the device at every
 * point of an axis-aligned lattice, on demand.  Point (i, j, k), i < count[0], j < count[1],
 * k < count[2], lies at origin + (i spacing[0], j spacing[1], k spacing[2]) (each product and sum
 * rounded, no contraction), wrapped into the periodic domain like a particle; points outside the
 * domain are legal and wrap.  2-D: z is ignored and count[2] must be 1.
 *
 * Per point, over the particles j of the selected classes within `radius` h of it: r the exact FP64
 * minimum-image distance to the position PressureP was computed at (the last step's sorted set: the
 * wrapped position before that step's motion), w = (1 - r/h)^2 for r < h, and MPH_SAMPLE_CHANNELS
 * doubles (MphSampleChannel): COUNT the contributing particles, WSUM = sum w (the fill level: 0 in
 * empty space), P = sum w PressureP / sum w with the last step's PressureP, VX VY VZ = sum w v /
 * sum w with v the velocity that step started from: what mph_get(MPH_FIELD_VELOCITY) returned
 * before the step, except where the step's own preamble rewrites it first: the Turek_Hron inlet
 * profile on its fluid particles, and calculateWall on the wall particles (their velocity and
 * position are set from the wall motion before the sort; a static wall keeps its velocity 0 and its
 * position to the last bit or two).  No contributor: all six are 0.
 * out is [count[2]][count[1]][count[0]][MPH_SAMPLE_CHANNELS], i fastest.
 * A point's six values depend only on the point, the radius, the class mask and the state -- not on
 * the lattice around it -- and the same call gives the same bits again.                          */
#define MPH_SAMPLE_CHANNELS   6
#define MPH_SAMPLE_MAX_POINTS (1 << 24)
typedef enum MphSampleChannel {
    MPH_SAMPLE_COUNT = 0,
    MPH_SAMPLE_WSUM = 1,
    MPH_SAMPLE_P = 2,
    MPH_SAMPLE_VX = 3,
    MPH_SAMPLE_VY = 4,
    MPH_SAMPLE_VZ = 5
} MphSampleChannel;
typedef struct MphSampleGrid {
    double origin[3];
    double spacing[3];     /* > 0 */
    int count[3];          /* >= 1 each, count[0] count[1] count[2] <= MPH_SAMPLE_MAX_POINTS */
    int classes;           /* bit mask: 1 fluid (types 0, 1), 2 structure (2, 3), 4 walls (4, 5); 0: fluid only */
    double radius;         /* 0: RadiusRatioP * dx; must be <= MaxRadius + MARGIN (the cell stencil's reach) */
} MphSampleGrid;           /* 72 bytes: origin 0, spacing 24, count 48, classes 60, radius 64 */
/* Sample the lattice *g into host memory `out`.  A flush point like mph_get; it changes no state and
 * touches no step graph.  MPH_ERR_ARG: no step since creation or since the last mph_set (the sorted
 * set is not that state's), a count or spacing <= 0, more than MPH_SAMPLE_MAX_POINTS points, a radius
 * below 0 or over the stencil's reach, class bits above 7, count[2] != 1 in 2-D.
 * MPH_ERR_UNSUPPORTED: slab mode.  A context without particles gives zeros.                        */
int mph_sample_grid(MphCtx* ctx, const MphSampleGrid* g, double* out);
/* mph_sample_grid with the kernel timed through the profiler of mph_profile_steps: *kernel_ms (may
 * be NULL) receives its duration from HIP events, name32 (32 chars, may be NULL) the name it was
 * recorded under (empty where no kernel ran: a context without particles).                        */
int mph_sample_grid_timed(MphCtx* ctx, const MphSampleGrid* g, double* out, double* kernel_ms, char* name32);
/* VTK XML ImageData (.vti) of a sampled lattice, host only: WholeExtent 0 nx-1 0 ny-1 0 nz-1, Origin
 * and Spacing of *g, Float64 point arrays Count, WSum, PressureP and Velocity (3 components) in raw
 * appended data (UInt64 headers), the doubles as sampled.                                         */
int mph_write_vti_arrays(const char* path, const MphSampleGrid* g, const double* out);

/* ---- free-surface gauges ---------------------------------------------------------------------- */

/* The water level H(t) at gauge stations, inside the per-step monitors, and as an elevation map on
 * demand.  A gauge is a straight line parallel to coordinate axis `axis` through a point whose
 * coordinate along that axis is ignored (2-D: its z too, and the axis is 0 or 1).  Its particles are
 * the fluid particles (types 0, 1) of the last step's sorted set -- the wrapped positions before
 * that step's motion, the ones PressureP was computed at, as for the probes -- whose distance r from
 * the line is below the radius h: r the minimum-image distance over the dim - 1 other axes, from
 * the gauge point wrapped into the periodic domain like a particle, r = sqrt(q0 q0 [+ q1 q1]) with
 * the lower axis first, FP64, no contraction.  Per gauge MPH_GAUGE_CHANNELS doubles
 * (MphGaugeChannel): COUNT of these particles; TOP, their largest coordinate along the axis (-inf
 * with none; spray counts); BOTTOM, the smallest (+inf with none); WET, the number of distinct
 * occupied bins along the axis (0 with none), a particle's bin being
 *     min(max((int)floor((x - domain_min[axis]) / particle_spacing), 0), nbins - 1),
 *     nbins = (int)ceil((domain_max[axis] - domain_min[axis]) / particle_spacing)
 * (FP64, IEEE division): WET * particle_spacing is the wetted length a wire gauge reads, whatever
 * droplets fly above the surface.  All four are order-independent, hence bit-exact functions of the
 * state, the gauge and the radius: the same in any batch shape, beside any other gauges, from the
 * monitors or from the map.  nbins must be <= MPH_GAUGE_MAX_BINS.                               */
#define MPH_GAUGE_MAX            64
#define MPH_GAUGE_CHANNELS       4
#define MPH_GAUGE_MAX_BINS       8192
#define MPH_GAUGE_GRID_MAX_LINES (1 << 20)
typedef enum MphGaugeChannel { MPH_GAUGE_COUNT = 0, MPH_GAUGE_TOP = 1, MPH_GAUGE_BOTTOM = 2, MPH_GAUGE_WET = 3 } MphGaugeChannel;

typedef struct MphGaugeConfig {      /* 24 bytes: axis 0, ngauge 4, points 8, radius 16 */
    int axis;              /* 0, 1, 2 (2-D: 0, 1); -1: the axis of the largest |gravity| component
                              (ties: the lowest axis; zero gravity: MPH_ERR_ARG) */
    int ngauge;            /* 0..MPH_GAUGE_MAX */
    const double* points;  /* [ngauge][3] */
    double radius;         /* 0: RadiusRatioP * dx; must be <= MaxRadius + MARGIN (the cell stencil's reach) */
} MphGaugeConfig;
/* Set the gauges of the monitors that are on (cfg == NULL or ngauge == 0: none).  A reconfiguration
 * like mph_monitor_configure: a flush point, the ring is emptied, STEP counts from this call, the
 * step graphs are captured again at the next step.  A sample is then head, tracked rows, probes and
 * {COUNT, TOP, BOTTOM, WET} per gauge: mph_monitor_sample_doubles returns MPH_MONITOR_HEAD +
 * 6 ntrack + 2 nprobe + MPH_GAUGE_CHANNELS ngauge.  mph_monitor_configure replaces the whole
 * configuration: after it there are no gauges.  MPH_ERR_ARG: monitors off, a count over the maximum,
 * a bad axis, a radius below 0 or over the stencil's reach, too many bins.  MPH_ERR_UNSUPPORTED: slab
 * mode.                                                                                           */
int mph_gauge_configure(MphCtx* ctx, const MphGaugeConfig* cfg);

typedef struct MphGaugeGrid {        /* 72 bytes: origin 0, spacing 24, count 48, axis 60, radius 64 */
    double origin[3]; double spacing[3]; int count[3]; int axis; double radius;
} MphGaugeGrid;
/* The elevation map on demand: the record of every line of a lattice.  Line (i, j, k) passes through
 * origin + (i spacing[0], j spacing[1], k spacing[2]) (each product and sum rounded, no contraction;
 * lines outside the domain wrap); count[axis] must be 1, and count[2] in 2-D; at most
 * MPH_GAUGE_GRID_MAX_LINES lines; a spacing must be > 0 where its count is above 1.  The axis and
 * radius rules are mph_gauge_configure's.  out is [count[2]][count[1]][count[0]][MPH_GAUGE_CHANNELS],
 * i fastest.  A flush point, legal where mph_sample_grid is (MPH_ERR_ARG before the first step and
 * after mph_set, MPH_ERR_UNSUPPORTED in slab mode); it changes no state and touches no step graph.  A
 * context without particles gives {0, -inf, +inf, 0} for every line.                              */
int mph_gauge_grid(MphCtx* ctx, const MphGaugeGrid* g, double* out);

/* ---- lattice sampling and elevation maps on slab ranks ----------------------------------------- */

/* mph_sample_grid and mph_gauge_grid for a slab context (mph_create_slab and its kin); the calls above
 * keep refusing one.  A lattice is axis-aligned, so the rank that evaluates a point -- the one whose
 * slab holds the point's coordinate along the slab axis, wrapped like a particle's -- depends only on
 * the point's index along that axis: a rank owns planes of the lattice (mph_slab_lattice_owner with the
 * context's cuts), several runs of them where the lattice crosses the periodic seam or is longer than
 * the domain.  The owner evaluates a point over its sorted set, owned particles and ghosts: the radius
 * limit MaxRadius + MARGIN is below the halo width, so that set holds every contributor.  Additive: no
 * change of MPH_ABI_VERSION.  All of these return MPH_ERR_UNSUPPORTED on a single context and follow
 * the argument rules of the single-context calls, "no step since creation or since the last mph_set"
 * included; none changes the state or touches a step graph.
 *
 * This rank's part of the lattice *g, no communication: out has the layout of mph_sample_grid for the
 * whole lattice, and the rank writes the rows of the planes it owns and leaves every other row
 * untouched (the convention of mph_get in slab mode); only those planes are computed on the device
 * and copied from it.  *owned_points (may be NULL) receives the number of points written; 0 is legal.
 * The definition is mph_sample_grid's: COUNT is exact, the sums are taken in the rank's own cell order
 * (they differ from a single context's by reassociation only), the same call gives the same bits.   */
int mph_dist_sample_grid_partial(MphCtx* ctx, const MphSampleGrid* g, double* out, long long* owned_points);
/* Collective: every rank calls it with the same *g; the ranks' planes travel to rank 0, which receives
 * the whole lattice in out -- bit for bit the merge of the partial calls.  The other ranks may pass
 * out == NULL.  MPH_ERR_TRANSPORT where the gather fails.                                           */
int mph_dist_sample_grid(MphCtx* ctx, const MphSampleGrid* g, double* out);

/* A rank's record of a line: {COUNT, TOP, BOTTOM, WET, LOBIN, HIBIN}, LOBIN and HIBIN the lowest and
 * highest occupied bin (-1 with none).
 *   A line not parallel to the slab axis lies in one plane: the owner of the plane computes it over
 *   its owned particles and its ghosts (every particle within the radius across is among them); every
 *   other rank's record is {-1, -inf, +inf, 0, -1, -1}.
 *   A line parallel to the slab axis runs through every rank (count[axis] is 1 there): every rank
 *   computes every line over the fluid particles it owns, along the whole extent of its window.      */
#define MPH_DIST_GAUGE_RECORD 6
/* This rank's records of every line of *g, records [count[2]][count[1]][count[0]][MPH_DIST_GAUGE_RECORD];
 * no communication.                                                                                  */
int mph_dist_gauge_grid_partial(MphCtx* ctx, const MphGaugeGrid* g, double* records);
/* The ranks' records made a map: records[r] is rank r's [nlines][MPH_DIST_GAUGE_RECORD], out receives
 * [nlines][MPH_GAUGE_CHANNELS], the layout of mph_gauge_grid.  Host only, no context.  Per line, over
 * the ranks with COUNT >= 0 in rank order: COUNT is the sum, TOP the maximum, BOTTOM the minimum; WET is
 * the sum of the ranks' WET minus one for every pair of consecutive non-empty ranks (COUNT > 0) whose
 * HIBIN == LOBIN.  An owned fluid particle lies in its rank's slab and the bin does not decrease with
 * the coordinate, so the ranks' bins are ordered and only such a pair can share one (a bin shared by
 * three ranks is counted three times and subtracted twice).  Every channel is an integer count, an
 * extremum or a population: the map is a bit-exact function of the state, the same as a single
 * context's.  MPH_ERR_ARG: a line with no rank at COUNT >= 0, nranks < 1, nlines < 0, a null pointer. */
int mph_gauge_combine(int nranks, long long nlines, const double* const* records, double* out);
/* Collective: every rank calls it with the same *g; rank 0 gathers the ranks' records, combines them
 * and receives the map in out ([count[2]][count[1]][count[0]][MPH_GAUGE_CHANNELS]); the other ranks may
 * pass out == NULL.  MPH_ERR_TRANSPORT where the gather fails.                                      */
int mph_dist_gauge_grid(MphCtx* ctx, const MphGaugeGrid* g, double* out);

/* ---- particle selections ---------------------------------------------------------------------- */

/* A selection is a subset of the particles, built on the device on demand: read any field for the
 * subset only, write a frame of the subset only, reduce load, momentum and extent over it -- without
 * copying a whole array.  A context holds one selection: the selected original indices, ascending,
 * and each one's place in the sorted device arrays.  It is a snapshot of the current state: the next
 * mph_step, mph_set or mph_set_initial_velocity_profile makes it stale, and every consumer below
 * then returns MPH_ERR_ARG until the next mph_select (as it does before the first one).  Single
 * contexts only: every context entry point returns MPH_ERR_UNSUPPORTED in slab mode (slab ranks:
 * the mph_dist_* calls below).  Additive: no change of MPH_ABI_VERSION.
 *
 * Particle i of type t is selected iff all of: type_mask is 0 or has bit t; i % every == phase; box
 * is 0, or lo[d] <= x[d] < hi[d] on every axis d < dim (2-D: z is ignored) for x the particle's
 * Position as mph_get returns it now (box 1) or its InitialPosition (box 2: a body, wherever it has
 * moved).  The compares are raw: no periodic wrap, and a NaN coordinate or bound is never inside.   */
typedef struct MphSelection {   /* 64 bytes: type_mask 0, box 4, every 8, phase 12, lo 16, hi 40 */
    int type_mask;   /* bit t = particle type t (0..5); 0 = every type */
    int box;         /* 0 none, 1 on Position (as mph_get returns it now), 2 on InitialPosition */
    int every, phase;/* keep original index i iff i % every == phase; every >= 1, 0 <= phase < every */
    double lo[3], hi[3]; /* lo[d] <= x[d] < hi[d] for d < dim (2-D: z ignored); raw compare, no wrap; NaN never in */
} MphSelection;
/* Host only: *out from "types=0,1;box=x0,y0,z0,x1,y1,z1;on=initial;every=4;phase=1" -- any subset
 * of the keys in any order, separated by ';'; on=position (the default) or on=initial says what the
 * box tests and needs a box; without keys: every particle.  MPH_ERR_ARG on anything else (an unknown
 * key, a key twice, a wrong count of numbers, a type outside 0..5, every < 1, a phase outside
 * [0, every), trailing characters).                                                                */
int mph_selection_parse(const char* text, MphSelection* out);
/* Host only: 1 if particle `index` of type `type` at Position pos / InitialPosition pos0 is selected,
 * else 0 (the very function the device evaluates); MPH_ERR_ARG for every < 1, a phase outside
 * [0, every), box outside 0..2, mask bits above 0x3f, lo[d] > hi[d] (or a NaN bound) on an axis
 * d < dim of a box, dim not 2 or 3.  pos / pos0 may be NULL where the box does not read them.       */
int mph_selection_accepts(const MphSelection* s, int dim, int index, int type, const double pos[3],
                          const double pos0[3]);
/* sizeof(MphSelection) and the offsets of its six members as compiled into the library (out7).     */
int mph_selection_layout(int out7[7]);

/* Make *s the context's selection, evaluated on the current state, and return its size in *count
 * (may be NULL; 0 is a legal size).  A flush point like mph_get; legal before the first step.
 * MPH_ERR_ARG for what mph_selection_accepts refuses; a refused call leaves the selection made
 * before it as it was.                                                                             */
int mph_select(MphCtx* ctx, const MphSelection* s, int* count);
/* The selected original indices, ascending: `count` ints.                                          */
int mph_selected_ids(MphCtx* ctx, int* out);
/* mph_get for the selection: row r of out is, bit for bit, row ids[r] of what mph_get(field) returns
 * now, with the same widths (double[count][3], double[count], int[count], double[count][3][3]).
 * The sorted device arrays are gathered on the device and only the `count` rows are copied.         */
int mph_get_selected(MphCtx* ctx, int field, void* out);
/* Sums and extrema over the selection, reduced on the device: MPH_TOTALS doubles (MphTotalSlot), of
 * x = Position, v = Velocity, F = Force as mph_get returns them now and m = MPH_FIELD_MASS.
 * v.v = vx vx + vy vy + vz vz, left to right, no contraction; KE adds (0.5 m)(v.v); the torque adds
 * (x - c) x F with d = x - c a plain difference -- NO minimum image: take a centre on the same side
 * of a periodic face as the body; each component is d_a F_b - d_b F_a, two rounded products and
 * their rounded difference.  Empty selection: sums 0, minima +inf, maxima -inf, VMAX2 0.
 * The terms are added in an order fixed by `count` alone, over ascending original index (fixed
 * blocks of ranks, a wave fold, the blocks in order; no floating-point atomics), so the totals are a
 * bit-exact function of the state, the selection and c -- whatever the sorted order, the list format
 * or the batch shape that led to the state.
 * What Force holds, hence what a "load" is: for a fluid particle the step's total force; for a
 * structure particle the interface force plus gravity, zero on clamped particles; for a wall
 * particle the pair forces from every neighbour, which the reference computes and never applies.
 * Force is the LAST SUCCESSFUL mph_step's (stored by a call's last step; zeros or the creation's
 * values before the first): a load of step k needs an mph_step call that ends at step k.           */
#define MPH_TOTALS 24
typedef enum MphTotalSlot {
    MPH_TOT_COUNT = 0,           /* selected particles */
    MPH_TOT_MASS = 1,            /* sum m */
    MPH_TOT_PX = 2, MPH_TOT_PY = 3, MPH_TOT_PZ = 4,      /* sum m v */
    MPH_TOT_KE = 5,              /* sum (0.5 m)(v.v) */
    MPH_TOT_FX = 6, MPH_TOT_FY = 7, MPH_TOT_FZ = 8,      /* sum Force */
    MPH_TOT_TX = 9, MPH_TOT_TY = 10, MPH_TOT_TZ = 11,    /* sum (x - c) x Force */
    MPH_TOT_MX = 12, MPH_TOT_MY = 13, MPH_TOT_MZ = 14,   /* sum m x */
    MPH_TOT_XMIN = 15, MPH_TOT_XMAX = 16, MPH_TOT_YMIN = 17, MPH_TOT_YMAX = 18,
    MPH_TOT_ZMIN = 19, MPH_TOT_ZMAX = 20,                /* extent */
    MPH_TOT_VMAX2 = 21,          /* max v.v */
    MPH_TOT_RESERVED0 = 22,      /* zero */
    MPH_TOT_RESERVED1 = 23
} MphTotalSlot;
int mph_selection_totals(MphCtx* ctx, const double center[3], double out[MPH_TOTALS]);
/* mph_write_vtk / mph_write_vtu of the selection alone: the gathered arrays handed to
 * mph_write_vtk_arrays / mph_write_vtu_arrays with n = count, so the file is exactly what those
 * writers give for mph_get(...)[ids].                                                              */
int mph_write_vtk_selected(MphCtx* ctx, const char* path);
int mph_write_vtu_selected(MphCtx* ctx, const char* path);
/* For measurement: mph_select(*s), mph_get_selected of Position, Velocity and PressureP, and
 * mph_selection_totals(center), with every kernel launch timed through the profiler of
 * mph_profile_steps: ms[k] and names32 (32 chars each) receive launch k's duration from HIP events
 * and the name it was recorded under, for the first `max` launches; returns the number of launches.
 * The selection it made stays the context's.                                                       */
int mph_select_profile(MphCtx* ctx, const MphSelection* s, const double center[3], int max, double* ms,
                       char* names32);

/* ---- particle selections on slab ranks ---------------------------------------------------------- */

/* Selections for a slab context (mph_create_slab and its kin); the calls above keep refusing one.  A
 * rank's selection is the subset of the particles IT OWNS NOW -- what mph_owned_ids lists; a ghost is
 * never selected -- that the predicate of MphSelection accepts, held as ascending original indices of
 * the whole problem ([0, n) of mph_particle_count).  Position is what mph_get returns on the rank.
 * Ownership is a partition, so the ranks' selections partition the whole problem's: a box that spans a
 * cut or the periodic face selects each particle exactly once, on the rank that owns it.  The argument
 * rules, the snapshot rule (stale after mph_step, mph_set or mph_set_initial_velocity_profile: the
 * consumers then return MPH_ERR_ARG) and the legality before the first step are the single context's.
 * Additive: no change of MPH_ABI_VERSION.  Every context call below returns MPH_ERR_UNSUPPORTED on a
 * single context; none changes the state or touches a step graph, and no rank waits for another except
 * inside the calls named collective.
 *
 * Make *s this rank's selection and return its size in *count (may be NULL; 0 is legal).  No
 * communication; a flush point.  A refused call leaves the selection made before it as it was.
 * Property comes from the device, so a rank created from its own window (MphSlabOptions.ids) selects a
 * particle that came from outside it like any other; only a box on InitialPosition (box 2) needs the
 * static inputs: MPH_ERR_ARG where the rank owns a particle without them that the rest of *s accepts.
 * Memory: 12 bytes per particle of the WHOLE problem per rank (the flags and the two slot maps are
 * indexed by original index, which keeps the rows ascending without a sort on the device).         */
int mph_dist_select(MphCtx* ctx, const MphSelection* s, int* count);
/* This rank's selected original indices, ascending: `count` ints.  No communication.               */
int mph_dist_selected_ids(MphCtx* ctx, int* out);
/* Row r of out is, bit for bit, row ids[r] of what mph_get(field) fills on this rank, with the same
 * widths; the sorted device arrays are gathered on the device and only `count` rows are copied.
 * Property, Mass, Lambda, Mu and Kappa's modulus follow the device's type array.  MPH_ERR_ARG for
 * InitialPosition where a selected particle has no static inputs on this rank.  No communication.  */
int mph_dist_get_selected(MphCtx* ctx, int field, void* out);
/* mph_selection_totals over this rank's selection: the same terms in the same fixed order (blocks of
 * 1,024 ranks over ascending original index, the wave fold, the records in order), so a rank's record
 * is a bit-exact function of the state, the selection, the centre and the cuts.  An empty selection
 * gives the identities (sums 0, minima +inf, maxima -inf, VMAX2 0).  No communication.             */
int mph_dist_selection_totals_partial(MphCtx* ctx, const double center[3], double out[MPH_TOTALS]);
/* The ranks' records made one: records[r] is rank r's MPH_TOTALS doubles.  Host only, no context.
 * Rank 0's record is combined with ranks 1, 2, ... in order, in plain FP64 without contraction: COUNT
 * and the sums (MASS, P*, KE, F*, T*, M*) add, the minima take the minimum, the maxima and VMAX2 the
 * maximum, the reserved slots are 0.  The result is a function of the records and of the rank order,
 * bit for bit.  MPH_ERR_ARG: nranks < 1, a null pointer.                                           */
int mph_totals_combine(int nranks, const double* const* records, double out[MPH_TOTALS]);
/* Collective (every rank calls it with the same centre): rank 0 gathers the partial records and
 * receives mph_totals_combine of them in out, bit for bit; the other ranks may pass out == NULL.
 * MPH_ERR_TRANSPORT where the gather fails.                                                        */
int mph_dist_selection_totals(MphCtx* ctx, const double center[3], double out[MPH_TOTALS]);
/* Collective (every rank, the same field): rank 0 receives every rank's rows of
 * mph_dist_get_selected(field) merged by ascending original index in out, the indices in ids, and
 * returns the number of rows; MPH_ERR_ARG on rank 0 when cap_rows (the rows out and ids hold) is too
 * small -- mph_particle_count always suffices.  The other ranks return 0 and may pass NULL with
 * cap_rows == 0.  Only selected rows travel.  MPH_ERR_TRANSPORT where the gather fails, or on rank 0
 * where another rank could not read its rows.                                                       */
long long mph_dist_gather_selected(MphCtx* ctx, int field, void* out, int* ids, long long cap_rows);
/* Collective: rank 0 writes exactly what mph_write_vtk_arrays / mph_write_vtu_arrays give for the
 * merged selected rows, n the total count.  Every rank gathers its selected rows on the device; none
 * fetches a whole array, and rank 0 builds no array of the whole problem's length (unlike
 * mph_write_vtk on a slab context).  Needs static inputs for every selected particle (InitialPosition). */
int mph_dist_write_vtk_selected(MphCtx* ctx, const char* path);
int mph_dist_write_vtu_selected(MphCtx* ctx, const char* path);

/* ---- velocity gradient, vorticity and free-surface fields ------------------------------------- */

/* Per-particle fields derived from the state on demand, by one pass over the step's neighbour lists:
 * the velocity gradient with divergence, vorticity and shear rate, and a free-surface marker.  Per
 * particle MPH_KIN_CHANNELS doubles (MphKinChannel), read whole, for the current selection, or
 * written as a .vtu.  Single contexts only: every context entry point returns MPH_ERR_UNSUPPORTED in
 * slab mode.  Additive: no change of MPH_ABI_VERSION and no new MphField value.
 *
 * Inputs.  For particle i of any type, x_i and v_i are Position and Velocity as mph_get returns them
 * now (the set mph_compute_virial reads: the integrated set in list order after a step, the sorted
 * set before the first step).
 * Neighbours: the particles j != i of the classes in `classes` with r < h.  classes is the sampler's
 * mask (1 fluid: types 0, 1; 2 structure: 2, 3; 4 walls: 4, 5); 0 means all three.  The mask filters
 * neighbours only: every particle i gets a record.  q is the minimum image of x_j - x_i (the
 * reference's Mod(d + w/2, w) - w/2 per axis; 2-D: q_z = 0), r^2 = q_x q_x + q_y q_y + q_z q_z,
 * r = sqrt(r^2), w = (1 - r/h)^2 -- the weight of the probes and the sampler.  FP64, IEEE division
 * and square root, products left to right, no contraction.
 * Sums over those j, each in the order of the particle's list (the host function: j ascending):
 *   COUNT, WSUM = sum w, c_a = sum w q_a, G_ab = sum (w (v_j,a - v_i,a)) q_b,
 *   M_ab = sum (w q_a) q_b for a <= b, and M_ba = M_ab.
 * Channels:
 *   COUNT; WSUM; FILL = WSUM / n0(h), n0(h) the same sum w over a full lattice of spacing
 *   particle_spacing in dim dimensions, centre excluded (mph_kinematics_n0);
 *   CX CY CZ = c / WSUM, the offset of the neighbourhood's weighted centroid (0 with no neighbour;
 *   -C/|C| is the outward surface normal);
 *   L[a][b], row-major, dv_a/dx_b: L = G M^-1 on the dim x dim block by the closed-form adjugate,
 *     3-D: A00 = M11 M22 - M12 M12, A01 = M02 M12 - M01 M22, A02 = M01 M12 - M02 M11,
 *          A11 = M00 M22 - M02 M02, A12 = M01 M02 - M00 M12, A22 = M00 M11 - M01 M01 (A symmetric),
 *          det = M00 A00 + M01 A01 + M02 A02;   2-D: A00 = M11, A01 = -M01, A11 = M00,
 *          det = M00 M11 - M01 M01;   L_ab = (G_a0 A_0b + G_a1 A_1b [+ G_a2 A_2b]) / det,
 *     every sum left to right; in 2-D the z row and column are 0;
 *   DIV = L00 + L11 [+ L22]; WX WY WZ = (L21 - L12, L02 - L20, L10 - L01);
 *   SHEAR = sqrt(2 sum D_ab^2), D_ab = 0.5 (L_ab + L_ba), the nine squares added row-major;
 *   FLAGS as a double: bit 1 degenerate -- COUNT < dim + 1, or not det > det_floor (tr M / dim)^dim
 *   (the power as repeated products); then L, DIV, W and SHEAR are 0 -- bit 2 surface, FILL <
 *   surface_beta; bit 4, COUNT = 0;   the last three channels are reserved, zero.
 * The corrected gradient G M^-1 is what the elastic solid's Normalizer does: it returns a linear
 * velocity field's matrix exactly (to rounding), at a free surface and off the lattice alike.
 *
 * Radius: h <= MaxRadius, not MaxRadius + MARGIN.  After a step the pass repeats the step's search
 * storing every neighbour (as mph_compute_virial does), over the positions the step started from: a
 * pair within MaxRadius now was within MaxRadius + MARGIN then -- the reference's own assumption for
 * its virial.  Before the first step the lists are the state's own.                                 */
#define MPH_KIN_CHANNELS 24
typedef enum MphKinChannel {
    MPH_KIN_COUNT = 0, MPH_KIN_WSUM = 1, MPH_KIN_FILL = 2,
    MPH_KIN_CX = 3, MPH_KIN_CY = 4, MPH_KIN_CZ = 5,
    MPH_KIN_L = 6,               /* 6..14: L[a][b] at MPH_KIN_L + 3 a + b */
    MPH_KIN_DIV = 15,
    MPH_KIN_WX = 16, MPH_KIN_WY = 17, MPH_KIN_WZ = 18,
    MPH_KIN_SHEAR = 19,
    MPH_KIN_FLAGS = 20,          /* 1 degenerate | 2 surface | 4 no neighbour */
    MPH_KIN_RESERVED0 = 21, MPH_KIN_RESERVED1 = 22, MPH_KIN_RESERVED2 = 23
} MphKinChannel;
#define MPH_KIN_FLAG_DEGENERATE 1
#define MPH_KIN_FLAG_SURFACE    2
#define MPH_KIN_FLAG_ALONE      4
typedef struct MphKinematics {   /* 32 bytes: radius 0, surface_beta 8, det_floor 16, classes 24, reserved 28 */
    double radius;        /* 0: RadiusRatioV * dx; must be > 0 and <= MaxRadius */
    double surface_beta;  /* 0: 0.97 (the usual MPS number-density criterion); must be >= 0 */
    double det_floor;     /* 0: 1e-6; scale-free conditioning floor; must be >= 0 and < 1 */
    int classes, reserved;/* classes 0..7; reserved must be 0 */
} MphKinematics;
/* Host only: sizeof(MphKinematics) and the offsets of its five members as compiled (out6).         */
int mph_kinematics_layout(int out6[6]);
/* Host only: *n0 = n0(radius) of the configuration (radius 0: RadiusRatioV * dx), the lattice sum
 * over ix, iy [, iz] ascending.  MPH_ERR_ARG: a radius below 0 or not finite, dim not 2 or 3.       */
int mph_kinematics_n0(const MphConfig* cfg, double radius, double* n0);
/* Host only: the record of every particle from arrays (property[n], pos[n][3], vel[n][3]) into
 * out[n][MPH_KIN_CHANNELS] by a plain double loop over j ascending with the minimum image -- the
 * definition above, the per-pair and finishing arithmetic being the very functions the device runs.
 * O(n^2): MPH_ERR_ARG above 65,536 particles, and for what mph_compute_kinematics refuses in *kin.
 * For tests and small cases.                                                                        */
int mph_kinematics_arrays(const MphConfig* cfg, const MphKinematics* kin, int n, const int* property,
                          const double* pos, const double* vel, double* out);
/* Host only: a .vtu of n records in the style of mph_write_vtu_arrays (raw appended data, UInt64
 * headers): Points (Float64, pos[n][3]), Property (Int32) and the Float64 arrays Count, Fill,
 * Centroid (3 components), VelocityGradient (9), Divergence, Vorticity (3), ShearRate, Flags, the
 * doubles as computed.                                                                             */
int mph_write_vtu_kinematics_arrays(const char* path, int n, const int* property, const double* pos,
                                    const double* kin);
/* Compute the records of every particle on the device and keep them in the context.  A flush point
 * like mph_get; legal before the first step; it changes no state a step reads.  MPH_ERR_ARG: a bad
 * member of *kin (a radius below 0 or above MaxRadius, surface_beta < 0, det_floor outside [0, 1),
 * class bits above 7, reserved != 0), and after any mph_set or mph_set_initial_velocity_profile
 * until the next step (the lists and the sorted set are not that state's).  The result is a
 * snapshot: the next mph_step or mph_set makes it stale, and the getters and writers below then
 * return MPH_ERR_ARG (as they do before the first mph_compute_kinematics).                          */
int mph_compute_kinematics(MphCtx* ctx, const MphKinematics* kin);
/* The snapshot in original order: out[n][MPH_KIN_CHANNELS].                                         */
int mph_get_kinematics(MphCtx* ctx, double* out);
/* The snapshot's rows of the current selection: out[count][MPH_KIN_CHANNELS], row r bit for bit row
 * ids[r] of mph_get_kinematics, gathered on the device (only the count rows are copied).
 * MPH_ERR_ARG without a current selection or a current snapshot.                                   */
int mph_get_kinematics_selected(MphCtx* ctx, double* out);
/* mph_write_vtu_kinematics_arrays of the snapshot with Position and Property: every particle, or the
 * current selection's rows (the file the array writer gives for those rows).                        */
int mph_write_vtu_kinematics(MphCtx* ctx, const char* path);
int mph_write_vtu_kinematics_selected(MphCtx* ctx, const char* path);
/* mph_compute_kinematics with the kernel timed through the profiler of mph_profile_steps, like
 * mph_sample_grid_timed: *kernel_ms (may be NULL) its duration from HIP events, name32 (32 chars,
 * may be NULL) the name it was recorded under (empty where no kernel ran).                         */
int mph_compute_kinematics_timed(MphCtx* ctx, const MphKinematics* kin, double* kernel_ms, char* name32);
/* Host only: *out from "radius=..;classes=..;beta=..;det=.." -- any subset of the keys in any order,
 * separated by ';'; empty text: the defaults (all members 0).  MPH_ERR_ARG on anything else (an
 * unknown key, a key twice, no number, a class mask that is no integer in 0..7).                    */
int mph_kinematics_parse(const char* text, MphKinematics* out);

/* ---- measurement ---------------------------------------------------------------------------- */

/* Run nsteps with a HIP event pair around every kernel launch (direct launches on the
 * context's stream, no graph) and report per-kernel-kind average duration in milliseconds.
 * names: MPH_PROFILE_MAX slots of 32 chars; returns the number of entries.  The last entry is
 * "gpu_busy": the union of all kernel intervals per step (launches = nsteps), which is less than
 * their sum where kernels of two streams overlap (slab mode).                                  */
#define MPH_PROFILE_MAX 24
int mph_profile_steps(MphCtx* ctx, int nsteps, double* avg_ms, int* launches, char* names32);
/* The list kernels as the timed steps run them (direct launches of mph_profile_steps take 3-8 %
 * longer): the search (with the XCD split), pass A and pass B, each captured `reps` (1..64) times
 * into a graph of its own and replayed between two HIP events on the context's stream; avg_ms3 =
 * milliseconds per launch (-1: not measured -- pass B with elastic slots).  Each replay recomputes
 * the last step's results bit for bit, so the state is unchanged (slab contexts: on the rank's
 * own set, no exchange, pass B as one launch).  After at least one step (else MPH_ERR_ARG).     */
int mph_profile_graphs(MphCtx* ctx, int reps, double* avg_ms3);
/* Phase timing: the reference's clock() buckets of its step loop (main.cpp:695-700) from HIP
 * events.  With on != 0 mph_step launches the kernels of its step batches directly instead of
 * replaying the captured graphs (HIP does not time events recorded inside a graph), with three
 * events per step -- before the cell sort, after the neighbour search, after the elastic
 * substeps -- read after every batch (mph_step returns after its steps have run anyway);
 * mph_compute_virial is bracketed too.  mph_phase_times adds up, in milliseconds of GPU time since the context was
 * created: [0] neighbour search (calculateNeighbor with its cell sort: k_prep .. k_neighbors),
 * [1] explicit calculation (the pass-A/pass-B sums, integration and elastic substeps), [2] the
 * virial.  Single contexts only (slab mode: MPH_ERR_ARG for on != 0).                          */
int mph_phase_timing(MphCtx* ctx, int on);
int mph_phase_times(const MphCtx* ctx, double* out3);
/* Mean/max neighbour count of the last step (for algorithmic byte/flop accounting).         */
int mph_neighbor_stats(MphCtx* ctx, double* mean, int* max);

/* ---- multi-GPU slab decomposition (one process per GPU, RCCL over xGMI) ------------------ */

/* The reference runs one process over all particles (OpenMP/OpenACC, main.cpp:597-686); it has
 * no domain decomposition.  These entry points add one: the periodic domain is cut into
 * `nranks` slabs along `axis` (equal widths, or the caller's cuts: MphSlabOptions.cuts); each rank
 * owns the particles inside its slab, mirrors the
 * ones within one cutoff of a face to that neighbour as ghosts, and hands particles that crossed
 * a face to the neighbour at the start of the next step.  Per step: one exchange of
 * (x, v, type, id) for migrants + ghosts before the cell sort, one of the pass-A values
 * (PressureP [, GravityCenter, PressureA]) of the ghosts before the force pass.
 * Elastic-solid particles (types 2, 3) are owned for good by the slab of their InitialPosition;
 * their fixed Lagrangian lists reach into static ghost slots of the two neighbours, refreshed
 * before each half of every elastic substep (displacements, then first Piola-Kirchhoff stress).
 *
 * mph_get in slab mode fills only the entries of the particles this rank owns (indexed by the
 * original particle index, arrays of mph_particle_count() = the global count); the other
 * entries are left untouched, so a caller can merge the ranks' arrays.                        */

/* 128-byte RCCL unique id generated on rank 0 and shared out of band by the caller.          */
int mph_dist_unique_id(char* out128);
/* Same as mph_create, but this rank owns only the particles whose slab (along `axis`) is
 * `rank` of `nranks`; all ranks pass the full particle set.  Transport: RCCL (ncclSend/Recv
 * with the two periodic neighbours, on the context's stream).  Every size of a step is kept on
 * the device and messages travel with fixed capacities of 1.25 c + 4096 particles for a count c
 * (checked every 32 steps, also inside one mph_step call, and grown when a count passed 90 %), so
 * the steps are replayed from captured hipGraphs with no host round trip in between
 * (MPH_SLAB_GRAPHS=0: direct launches).                                                       */
int mph_create_dist(MphCtx** ctx, const MphConfig* cfg, int n, const int* property,
                    const double* pos, const double* pos0, const double* vel, int device,
                    int rank, int nranks, const char* unique_id128, int axis);
/* Host-staged transport for the same protocol: the context copies each message to pinned host
 * memory and calls `fn`, which must deliver send_l to the left neighbour (received there as
 * its recv_r) and send_r to the right neighbour (its recv_l), with the byte counts given.
 * Used to run several ranks on one GPU (tests) or where RCCL is unavailable.  Returns 0 on
 * success.                                                                                     */
typedef int (*mph_host_exchange_fn)(void* user, const void* send_l, size_t bytes_send_l,
                                    const void* send_r, size_t bytes_send_r, void* recv_l,
                                    size_t bytes_recv_l, void* recv_r, size_t bytes_recv_r);
int mph_create_dist_host(MphCtx** ctx, const MphConfig* cfg, int n, const int* property,
                         const double* pos, const double* pos0, const double* vel, int device,
                         int rank, int nranks, int axis, mph_host_exchange_fn fn, void* user);
/* General slab-mode constructor: the transport (RCCL unique id, or a host exchange callback) and,
 * with n_glob > 0, slab-local creation -- the arrays hold only the n particles this rank needs,
 * with their original indices ids[n] (ascending) among n_glob: every particle whose coordinate
 * along the axis (Position; InitialPosition for elastic particles) lies within the window of
 * mph_slab_window.  Others are not needed (ghosts arrive from the neighbours).  In slab-local mode
 * mph_get returns the static inputs (Property, InitialPosition, Mass, ...) for the particles this
 * rank was created with, and the state for the particles it owns.                             */
typedef struct MphSlabOptions {
    int rank, nranks, axis;
    const char* unique_id128;          /* RCCL transport, or NULL and host_fn:                  */
    mph_host_exchange_fn host_fn;      /* host-staged transport                                  */
    void* host_user;
    int n_glob;                        /* 0: the arrays hold every particle (n == n_glob)       */
    const int* ids;
    /* NULL: nranks equal slabs; else the nranks - 1 interior boundaries along the axis, strictly
     * ascending inside the domain (slab r = [cuts[r-1], cuts[r]), the first and last reaching
     * the domain faces), the same array on every rank -- e.g. particle-count quantiles, so that
     * the ranks hold equal shares (balanced_cuts in particlemethod_fsi_amd/dist.py)           */
    const double* cuts;
} MphSlabOptions;
int mph_create_slab(MphCtx** ctx, const MphConfig* cfg, int n, const int* property, const double* pos,
                    const double* pos0, const double* vel, int device, const MphSlabOptions* opt);
/* Host-only: the periodic window [lo, hi) (out2) along `axis` that rank `rank` of `nranks` needs
 * at slab-local creation: its slab widened by two halo widths on each side.  cuts: as in
 * MphSlabOptions (NULL: equal slabs).                                                         */
int mph_slab_window(const MphConfig* cfg, int rank, int nranks, int axis, const double* cuts, double* out2);
/* One-rank RCCL communicator on `device` whose two neighbours are itself: checks that the
 * exchange delivers each message to the right buffer (the per-peer ordering nranks == 2 relies
 * on) without a second GPU.  Returns 0 on success.                                            */
int mph_dist_selftest(int device);
/* Slab-mode facts for reports: out8 = {slab ranks of the decomposition (1 without slabs), rank,
 * size of the RCCL communicator (ncclCommCount; 0 under the host-staged transport), steps
 * replayed from captured graphs,
 * local array capacity, largest send / receive message capacity (particles), particles held
 * (owned + ghosts)}.                                                                          */
int mph_dist_info(const MphCtx* ctx, int* out8);
/* Pass-B mode of a slab context (out5; all -1 without slabs): {overlap on (1) / off (0), how it
 * was set: 1 / 0 forced by MPH_SLAB_OVERLAP, -1 chosen at creation by the ranks together, then
 * the creation probe's maxima over ranks in ms -- halo exchange, redistribution exchange (both at
 * their message capacities), the cost of pass B split into interior and face launches over one
 * launch (-1: not probed)}.  Overlap is chosen when the two exchanges take longer than the split. */
int mph_dist_overlap(const MphCtx* ctx, double* out5);
/* Mean/max length of the stored neighbour lists of the last search (what the passes walk: the
 * pairs within the passes' largest radius; with MPH_LIST_FULL=1 at creation every
 * neighbour, = mph_neighbor_stats): entries, not rows (the gap rows of the aligned lists do not
 * count).  ABI 4 (round 6): replaces mph_list_formats, which reported the compact 16-bit list
 * format removed from the product.                                                            */
int mph_list_stats(MphCtx* ctx, double* mean, int* max);
/* How the last search laid the stored lists out in rows (the aligned rows of DESIGN.md 3.3), for
 * verification: out6 = {waves (tiles of 64 particles), waves that made at least one row jump,
 * row jumps in all, the most jumps of one wave, gap rows in all (the rows the lanes skipped at
 * their jumps), the most rows of one lane (entries + gaps)}.  Read-only, reduced on the host.
 * A wave with 16-bit rows (mph_list_format_stats) jumps at every stencil group end; only its jumps
 * that left a gap in some lane are counted, as a wave with 32-bit rows makes no other.
 * Single contexts only (MPH_ERR_UNSUPPORTED in slab mode).  ABI 5.                              */
int mph_list_layout(MphCtx* ctx, long long out6[6]);
/* Lazy wall steps, for verification: out2 = {idle wave-steps, lazy steps} since the
 * creation.  A lazy step is a step that stores no output-only field (every step of an 8-step batch
 * or of a call's remainder but the last) in a single context without monitors; on it the search
 * skips, and counts as idle, every wave of wall particles that no fluid or structure particle can
 * reach.  Both stay 0 in slab mode, with monitors configured, or with MPH_LAZY_WALLS=0 in the
 * environment at creation.  A flush point.  Additive: no change of MPH_ABI_VERSION.            */
int mph_idle_wall_stats(MphCtx* ctx, long long out2[2]);
/* Lean steps, for verification: out2 = {steps whose search ran its lean form, steps
 * whose pass A did} since the creation.  A lean step is a lazy step (above) of a context created
 * without MPH_LEAN_STEPS=0: its search accepts only the pairs it stores and counts no
 * NeighborCount (not with MPH_LIST_FULL=1), its pass A leaves out the DensityA and GravityCenter
 * sums (not with surface tension, where pass B reads them).  Both stay 0 wherever no step is lazy.
 * A flush point.  Additive: no change of MPH_ABI_VERSION.                                        */
int mph_lean_step_stats(MphCtx* ctx, long long out2[2]);
/* The key fold, for verification: out2 = {steps whose pass B left the next step's
 * cell keys, steps that opened with a k_prep launch} since the creation.  Inside one replayed graph
 * (or one phase-timed or profiled batch) pass B moves and wraps the particles and computes the next
 * step's keys, slots and cell histogram before it stores them, so only the graph's first step
 * launches k_prep.  Single contexts without structure particles and without monitors, created
 * without MPH_KEY_FOLD=0; elsewhere the first stays 0 and the second counts every step.  A flush
 * point.  Additive: no change of MPH_ABI_VERSION.                                               */
int mph_key_fold_stats(MphCtx* ctx, long long out2[2]);
/* The formats of the neighbour lists, for verification: out3 = {waves whose rows are
 * 16-bit ones, waves with 32-bit rows, waves among the latter that began in the 16-bit format and
 * started over} of the last search.  A 3-D interior wave takes the 16-bit rows when the candidates
 * of each of its stencil groups lie within 8191 indices; none does in 2-D, in slab mode or with
 * MPH_LIST16=0 at creation.  A flush point.  Additive: no change of MPH_ABI_VERSION.            */
int mph_list_format_stats(MphCtx* ctx, long long out3[3]);
/* Of the waves with 32-bit rows of the last search, those that are interior 3-D waves turned away
 * by the span limit alone (the others are waves at periodic faces, idle wall waves, ghosts,
 * restarted waves): *out.  A flush point.  Additive: no change of MPH_ABI_VERSION.               */
int mph_list_span_misses(MphCtx* ctx, long long* out);
/* The same decision wave by wave, for verification: out holds 8 ints per wave (tile of 64 particles
 * in the last search's sorted order; mph_list_layout's out6[0] waves).  out[8 w] = 0: the wave
 * never decided (at a periodic face, idle walls, ghosts, 2-D, slab mode, MPH_LIST16=0), 1: 16-bit
 * rows, 2: it began in the 16-bit format and started over, 3: turned away by the span limit.
 * out[8 w + 1 .. 8 w + 7] = the seven group bases of a wave with 16-bit rows (sorted indices), else
 * 0.  Read-only, reduced on the host.  A flush point.  Additive: no change of MPH_ABI_VERSION.   */
int mph_list_wave_formats(MphCtx* ctx, int* out);
/* The neighbour lists of calculateNeighbor themselves (main.cpp:1764-1772: Neighbor[i][k] = j for
 * k < 512), for verification: the sets of the `count` particles [first, first + count) (original
 * order) from the last search, each row as ascending original indices (the reference's rows are in
 * its cell-scan order; the sets are what both define).  counts[count] receives each particle's
 * NeighborCount; ids the rows back to back (row k starts at the sum of min(counts, 512) before
 * it), ids_cap its capacity in ints.  Returns the number of ids written, or a negative MphStatus
 * (MPH_ERR_ARG when ids_cap is too small).  Single contexts with the reference's whole lists only
 * (created with MPH_LIST_FULL=1 in the environment: by default the lists keep only the pairs
 * within the largest radius of the passes' sums, NeighborCount still counts every neighbour;
 * MPH_ERR_UNSUPPORTED in slab mode or without MPH_LIST_FULL=1).  The gap rows of the aligned
 * lists are skipped.                                                          */
int mph_neighbor_rows(MphCtx* ctx, int first, int count, int* counts, int* ids, long long ids_cap);
/* Particles currently owned by this rank (after the last migration); their original indices.  */
int mph_owned_count(const MphCtx* ctx);
int mph_owned_ids(MphCtx* ctx, int* out_ids);
/* Host-only: the slab bounds [lo, hi) of `rank` and the halo width along `axis` that a slab
 * context would use (out3 = {lo, hi, h}), and which rank owns coordinate c.  cuts: as in
 * MphSlabOptions (NULL: equal slabs).                                                         */
int mph_slab_bounds(const MphConfig* cfg, int rank, int nranks, int axis, const double* cuts, double* out3);
int mph_slab_owner(const MphConfig* cfg, int nranks, int axis, const double* cuts, double c);
/* Host-only: the owners of the planes of an axis-aligned lattice along the slab axis.  owner[i], i <
 * count_a, is mph_slab_owner of origin_a + (double)i * spacing_a -- the product and the sum each
 * rounded, no contraction: the kernels' own expression -- wrapped into the periodic domain like a
 * particle's coordinate.  A lattice that crosses the periodic seam or is longer than the domain gives
 * a rank several runs of planes.  MPH_ERR_ARG: what mph_slab_owner refuses, count_a < 1, spacing_a <= 0,
 * a non-finite origin_a or spacing_a, owner NULL.  Additive: no change of MPH_ABI_VERSION.        */
int mph_slab_lattice_owner(const MphConfig* cfg, int nranks, int axis, const double* cuts, double origin_a,
                           double spacing_a, int count_a, int* owner);

#ifdef __cplusplus
}
#endif
#endif /* MPH_GPU_H_INCLUDED */
