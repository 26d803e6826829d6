// mph_main.cpp -- `mph_explicit`: drop-in replacement of the reference executable.
//
// Same command line as main.cpp:494-508:
//     mph_explicit <data> <grid> <prof pattern> <vtk pattern> <log> [nthreads] [device]
// Same driver semantics as main.cpp:528-700: read files, initialise, write output.vtk, then
// loop while Time < EndTime + 1e-5*Dt writing the .prof before a step (583-589) and the .vtk
// after a step (672-683).  Differences: the physics runs on MI355X through libmph_gpu.so;
// the .prof holds the current state (the OpenACC build writes stale host arrays);
// the timing report is wall time of the step loop, not clock() CPU time.  A <vtk pattern> ending
// in ".vtu" writes binary VTK XML files instead (mph_write_vtu).  MPH_MONITOR and
// MPH_SAMPLE add a time history and, per VTK output step, the fields on a lattice (below);
// MPH_OUTPUT_SELECT crops the VTK-step files to a particle selection and MPH_LOADS appends the
// totals of a selection -- the load on a body -- to a CSV every MPH_LOADS_STRIDE-th step (below;
// from slab ranks: MPH_DIST_OUTPUT_SELECT, MPH_DIST_LOADS);
// MPH_KINEMATICS writes the velocity gradient, vorticity and free-surface fields beside every VTK-step
// file (below).
//
// Several GPUs: MPH_SLABS=N runs the same case as N slab ranks (include/mph_gpu.h, one process
// per rank): the process forks N - 1 ranks before any HIP call, rank r takes device
// (device + r) mod the device count (MPH_SLAB_SHARE_DEVICE=1: all on `device`), the slabs lie
// along MPH_SLAB_AXIS (default z in 3-D, x in 2-D), the transport is RCCL (rank 0 makes the unique
// id and hands it to the others through pipes) or, with MPH_SLAB_TRANSPORT=host, neighbour
// exchanges over socket pairs.  Every output call is collective and rank 0 writes the files the
// single-GPU run writes, with the same cadence; MPH_DIST_MONITOR is MPH_MONITOR's time history from
// the ranks' combined records.
#include <fcntl.h>
#include <poll.h>
#include <signal.h>
#include <sys/prctl.h>
#include <sys/socket.h>
#include <sys/wait.h>
#include <unistd.h>

#include <cerrno>
#include <cmath>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>
#include <roctracer/roctx.h>

#include "../../include/mph_gpu.h"

static FILE* g_log = nullptr;

static bool g_quiet = false;   // slab ranks other than 0 report errors only

static void logf(const char* fmt, ...)
{
    if (g_quiet) return;
    va_list a, b;
    va_start(a, fmt);
    va_copy(b, a);
    if (g_log) vfprintf(g_log, fmt, a);
    vfprintf(stderr, fmt, b);
    va_end(a);
    va_end(b);
    if (g_log) fflush(g_log);
}

// ---- slab ranks: failure propagation ---------------------------------------------------------
// A rank that fails must not leave the others blocked in RCCL (no timeout there) or orphaned on
// their GPUs.  Children die with rank 0 (PR_SET_PDEATHSIG); rank 0 reaps children from a SIGCHLD
// handler and, on any non-zero or abnormal exit, kills the remaining ranks and exits 1 itself --
// from the handler, since rank 0 may be blocked inside a collective with the dead rank.
static constexpr int kMaxRanks = 64;
static pid_t g_child_pid[kMaxRanks];
static volatile sig_atomic_t g_child_done[kMaxRanks];   // 0 running, 1 exited 0, 2 failed
static volatile sig_atomic_t g_nchildren = 0;

static void kill_children()
{
    for (int k = 0; k < g_nchildren; ++k)
        if (g_child_done[k] == 0 && g_child_pid[k] > 0) kill(g_child_pid[k], SIGKILL);
}

static void on_sigchld(int)
{
    // only the registered ranks are reaped: any other child (a library's helper process) keeps its
    // exit status for its owner and cannot end the run
    const int saved = errno;
    for (int k = 0; k < g_nchildren; ++k) {
        if (g_child_done[k] != 0 || g_child_pid[k] <= 0) continue;
        int st = 0;
        if (waitpid(g_child_pid[k], &st, WNOHANG) != g_child_pid[k]) continue;
        const bool ok = WIFEXITED(st) && WEXITSTATUS(st) == 0;
        g_child_done[k] = ok ? 1 : 2;
        if (!ok) {
            static const char msg[] = "error: a slab rank failed; stopping the other ranks\n";
            (void)!write(2, msg, sizeof(msg) - 1);
            kill_children();
            _exit(1);
        }
    }
    errno = saved;
}

static void die(MphCtx* c, int rc, const char* what)
{
    g_quiet = false;
    logf("error: %s failed (%d): %s\n", what, rc, c ? mph_last_error(c) : "");
    kill_children();   // rank 0: the other ranks would wait for it forever (children: none)
    std::exit(1);
}

// ---- monitors: MPH_MONITOR=<csv path> -----------------------------------------------------------
// Opt-in time history (include/mph_gpu.h mph_monitor_*): every MPH_MONITOR_STRIDE-th step's sample
// -- sums, extrema, the particles MPH_MONITOR_TRACK=i,j,... and the pressure probes
// MPH_MONITOR_PROBES="x,y,z;x,y,z" -- is computed on the device inside the step graphs; the loop
// reads the ring after each batch of steps, where it synchronises anyway, and appends one CSV row
// per sample, a header line of column names first, the values as %.17g (the doubles round-trip).
struct MonitorCsv {
    FILE* f = nullptr;
    int stride = 1, width = 0;
    std::vector<int> track;
    std::vector<double> probes;
    std::vector<double> gauges;   // MPH_MONITOR_GAUGES: the gauge points, three numbers each
    std::vector<double> buf;
};

static std::vector<double> parse_numbers(const char* s)
{
    std::vector<double> v;
    while (s && *s) {
        char* e = nullptr;
        const double x = std::strtod(s, &e);
        if (e == s) { ++s; continue; }   // a separator (',' ';' blanks)
        v.push_back(x);
        s = e;
    }
    return v;
}

static void monitor_header(const MonitorCsv& m)
{
    static const char* cls[3] = {"fluid", "struct", "wall"};
    static const char* per[6] = {"count", "ke", "px", "py", "pz", "vmax2"};
    static const char* rest[12] = {"xmin", "xmax", "ymin", "ymax", "zmin", "zmax", "fluid_pmin", "fluid_pmax",
                                   "wall_pmax", "epot", "reserved0", "reserved1"};
    static const char* row[6] = {"x", "y", "z", "vx", "vy", "vz"};
    std::fprintf(m.f, "step,time");
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 6; ++k) std::fprintf(m.f, ",%s_%s", cls[c], per[k]);
    for (int k = 0; k < 12; ++k) std::fprintf(m.f, ",%s", rest[k]);
    for (int i : m.track)
        for (int k = 0; k < 6; ++k) std::fprintf(m.f, ",p%d_%s", i, row[k]);
    for (size_t q = 0; q < m.probes.size() / 3; ++q) std::fprintf(m.f, ",probe%zu_value,probe%zu_count", q, q);
    for (size_t q = 0; q < m.gauges.size() / 3; ++q)
        std::fprintf(m.f, ",gauge%zu_count,gauge%zu_top,gauge%zu_bottom,gauge%zu_wet", q, q, q, q);
    std::fprintf(m.f, "\n");
}

// ---- slab ranks: fork, socket-pair ring, RCCL id over pipes ----------------------------------

struct SlabRank {
    int rank = 0, nranks = 1;
    int left_fd = -1, right_fd = -1;   // host transport: the ring links to the two neighbours
    int uid_fd = -1;                   // RCCL: rank > 0 reads the unique id here
    std::vector<int> uid_out;          // rank 0 writes it to these
    std::vector<pid_t> children;
};

static bool write_all(int fd, const void* p, size_t n)
{
    const char* c = (const char*)p;
    while (n) {
        const ssize_t k = write(fd, c, n);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) return false;
        c += k;
        n -= (size_t)k;
    }
    return true;
}

static bool read_all(int fd, void* p, size_t n)
{
    char* c = (char*)p;
    while (n) {
        const ssize_t k = read(fd, c, n);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) return false;
        c += k;
        n -= (size_t)k;
    }
    return true;
}

// mph_host_exchange_fn over the two ring sockets: all four transfers progress together (poll), so
// two neighbours sending large messages to each other cannot block on full socket buffers
static int socket_exchange(void* user, const void* send_l, size_t bsl, const void* send_r, size_t bsr,
                           void* recv_l, size_t brl, void* recv_r, size_t brr)
{
    const SlabRank& R = *(const SlabRank*)user;
    const char* so[2] = {(const char*)send_l, (const char*)send_r};
    char* ri[2] = {(char*)recv_l, (char*)recv_r};
    size_t sn[2] = {bsl, bsr}, rn[2] = {brl, brr};
    const int fd[2] = {R.left_fd, R.right_fd};
    while (sn[0] || sn[1] || rn[0] || rn[1]) {
        pollfd pf[2];
        for (int k = 0; k < 2; ++k) {
            pf[k].fd = fd[k];
            pf[k].events = (short)((sn[k] ? POLLOUT : 0) | (rn[k] ? POLLIN : 0));
            pf[k].revents = 0;
        }
        if (poll(pf, 2, 600000) <= 0) return 1;   // 10 minutes without progress: a dead peer
        for (int k = 0; k < 2; ++k) {
            if (pf[k].revents & (POLLERR | POLLNVAL)) return 1;
            if (sn[k] && (pf[k].revents & POLLOUT)) {
                const ssize_t w = send(fd[k], so[k], sn[k], MSG_DONTWAIT | MSG_NOSIGNAL);
                if (w < 0 && errno != EAGAIN && errno != EINTR) return 1;
                if (w > 0) { so[k] += w; sn[k] -= (size_t)w; }
            }
            if (rn[k] && (pf[k].revents & (POLLIN | POLLHUP))) {
                const ssize_t r = recv(fd[k], ri[k], rn[k], MSG_DONTWAIT);
                if (r == 0) return 1;
                if (r < 0 && errno != EAGAIN && errno != EINTR) return 1;
                if (r > 0) { ri[k] += r; rn[k] -= (size_t)r; }
            }
        }
    }
    return 0;
}

// fork the ranks 1..N-1 (before anything touches the GPU); returns this process's rank
static int spawn_ranks(SlabRank& R, int n, bool host)
{
    R.nranks = n;
    std::vector<int> link(2 * n, -1);   // ring link k: rank k (right side) <-> rank k+1 (left side)
    if (host)
        for (int k = 0; k < n; ++k)
            if (socketpair(AF_UNIX, SOCK_STREAM, 0, &link[2 * k]) != 0) return -1;
    std::vector<int> pipes(2 * n, -1);
    if (!host)
        for (int r = 1; r < n; ++r)
            if (pipe(&pipes[2 * r]) != 0) return -1;
    std::fflush(nullptr);
    if (n > kMaxRanks) return -1;
    struct sigaction sa {};
    sa.sa_handler = on_sigchld;
    sigemptyset(&sa.sa_mask);
    sa.sa_flags = SA_RESTART | SA_NOCLDSTOP;
    if (sigaction(SIGCHLD, &sa, nullptr) != 0) return -1;
    // children are registered with SIGCHLD blocked, so the handler never sees a pid it cannot match
    sigset_t blk, old;
    sigemptyset(&blk);
    sigaddset(&blk, SIGCHLD);
    sigprocmask(SIG_BLOCK, &blk, &old);
    const pid_t parent = getpid();
    int me = 0;
    for (int r = 1; r < n; ++r) {
        const pid_t pid = fork();
        if (pid < 0) { sigprocmask(SIG_SETMASK, &old, nullptr); kill_children(); return -1; }
        if (pid == 0) {
            me = r;
            R.children.clear();
            g_nchildren = 0;
            signal(SIGCHLD, SIG_DFL);
            prctl(PR_SET_PDEATHSIG, SIGKILL);   // rank 0 gone: this rank goes too
            if (getppid() != parent) _exit(1);  // (it died before the line above)
            break;
        }
        R.children.push_back(pid);
        g_child_pid[g_nchildren] = pid;
        g_child_done[g_nchildren] = 0;
        g_nchildren = g_nchildren + 1;
    }
    sigprocmask(SIG_SETMASK, &old, nullptr);
    R.rank = me;
    if (host) {
        R.right_fd = link[2 * me];
        R.left_fd = link[2 * ((me + n - 1) % n) + 1];
        for (int k = 0; k < 2 * n; ++k)
            if (link[k] != R.right_fd && link[k] != R.left_fd) close(link[k]);
    } else {
        for (int r = 1; r < n; ++r) {
            if (me == 0) {
                R.uid_out.push_back(pipes[2 * r + 1]);
                close(pipes[2 * r]);
            } else if (r == me) {
                R.uid_fd = pipes[2 * r];
                close(pipes[2 * r + 1]);
            } else {
                close(pipes[2 * r]);
                close(pipes[2 * r + 1]);
            }
        }
    }
    return me;
}

int main(int argc, char** argv)
{
    std::string data = "sample.data", grid = "sample.grid", prof = "sample%03d.prof",
                vtk = "sample%03d.vtk", logname = "sample.log";
    int device = 0;
    if (argc > 1) data = argv[1];
    if (argc > 2) grid = argv[2];
    if (argc > 3) prof = argv[3];
    if (argc > 4) vtk = argv[4];
    if (argc > 5) logname = argv[5];
    // argv[6] is the reference's OpenMP thread count: accepted and ignored
    if (argc > 7) device = std::atoi(argv[7]);
    SlabRank R;
    const int nslabs = std::getenv("MPH_SLABS") ? std::atoi(std::getenv("MPH_SLABS")) : 1;
    const bool host_transport = std::getenv("MPH_SLAB_TRANSPORT") && std::strcmp(std::getenv("MPH_SLAB_TRANSPORT"), "host") == 0;
    if (nslabs > 1 && std::getenv("MPH_MONITOR"))   // (before any rank is started)
        die(nullptr, MPH_ERR_UNSUPPORTED, "MPH_MONITOR with MPH_SLABS > 1 (monitors need a single context; "
                                         "the slab ranks' combined samples: MPH_DIST_MONITOR)");
    if (nslabs <= 1 && std::getenv("MPH_DIST_MONITOR"))
        die(nullptr, MPH_ERR_ARG, "MPH_DIST_MONITOR needs MPH_SLABS > 1 (a single context: MPH_MONITOR)");
    if (nslabs > 1 && std::getenv("MPH_SAMPLE"))
        die(nullptr, MPH_ERR_UNSUPPORTED, "MPH_SAMPLE with MPH_SLABS > 1 (sampling needs a single context; "
                                         "the slab ranks' planes gathered: MPH_DIST_SAMPLE)");
    if (nslabs <= 1 && std::getenv("MPH_DIST_SAMPLE"))
        die(nullptr, MPH_ERR_ARG, "MPH_DIST_SAMPLE needs MPH_SLABS > 1 (a single context: MPH_SAMPLE)");
    if (nslabs > 1 && (std::getenv("MPH_OUTPUT_SELECT") || std::getenv("MPH_LOADS"))) {
        const std::string what = std::string(std::getenv("MPH_OUTPUT_SELECT") ? "MPH_OUTPUT_SELECT " : "") +
                                 (std::getenv("MPH_LOADS") ? "MPH_LOADS " : "") +
                                 "with MPH_SLABS > 1 (selections need a single context; the slab ranks' selections "
                                 "merged: MPH_DIST_OUTPUT_SELECT, MPH_DIST_LOADS)";
        die(nullptr, MPH_ERR_UNSUPPORTED, what.c_str());
    }
    if (nslabs <= 1 && std::getenv("MPH_DIST_OUTPUT_SELECT"))
        die(nullptr, MPH_ERR_ARG, "MPH_DIST_OUTPUT_SELECT needs MPH_SLABS > 1 (a single context: MPH_OUTPUT_SELECT)");
    if (nslabs <= 1 && std::getenv("MPH_DIST_LOADS"))
        die(nullptr, MPH_ERR_ARG, "MPH_DIST_LOADS needs MPH_SLABS > 1 (a single context: MPH_LOADS)");
    if (nslabs > 1 && std::getenv("MPH_KINEMATICS"))
        die(nullptr, MPH_ERR_UNSUPPORTED, "MPH_KINEMATICS with MPH_SLABS > 1 (kinematics need a single context)");
    if (nslabs > 1 && spawn_ranks(R, nslabs, host_transport) < 0) {
        std::fprintf(stderr, "error: could not start %d slab ranks\n", nslabs);
        return 1;
    }
    const bool root = R.rank == 0;
    g_quiet = !root;
    if (root) g_log = std::fopen(logname.c_str(), "w");
    {
        time_t t = time(nullptr);
        logf("start reading files at %s\n", ctime(&t));
    }
    MphConfig cfg;
    mph_config_default(&cfg, 2, MPH_MODULE_BAR);
    if (const char* d = std::getenv("MPH_DIM")) cfg.dim = std::atoi(d);
    if (const char* m = std::getenv("MPH_MODULE")) {
        // the module #define of main.cpp:54-59 by name (or MphModule number)
        static const char* names[] = {"bar", "dam", "turek_hron", "rolling1", "hydroelastic", "none"};
        cfg.module = std::atoi(m);
        for (int k = 0; k < 6; ++k)
            if (std::strcmp(m, names[k]) == 0) cfg.module = k;
    }
    // the `Rolling` wall-motion #define of main.cpp:58 (calculateWall 2974-3030)
    if (const char* w = std::getenv("MPH_WALL_MOTION"))
        cfg.wall_motion = std::strcmp(w, "rolling") == 0 ? MPH_WALL_ROLLING : std::atoi(w);
    int rc = mph_read_data_file(data.c_str(), &cfg);
    if (rc) die(nullptr, rc, "reading the data file");
    int n = 0;
    rc = mph_read_grid_header(grid.c_str(), &cfg, &n);
    if (rc) die(nullptr, rc, "reading the grid header");
    std::vector<int> prop(n);
    std::vector<double> pos(3 * (size_t)n), pos0(3 * (size_t)n), vel(3 * (size_t)n);
    rc = mph_read_grid_particles(grid.c_str(), n, prop.data(), pos.data(), pos0.data(), vel.data());
    if (rc) die(nullptr, rc, "reading the grid particles");
    int counts[3] = {0, 0, 0};
    for (int t : prop) counts[t < 2 ? 0 : (t < 4 ? 1 : 2)]++;
    if (root)
        std::printf("Fluid Particles: %d\nStructure Particles: %d\nWall Particles: %d\n", counts[0], counts[1], counts[2]);
    {
        time_t t = time(nullptr);
        logf("start initialization at %s\n", ctime(&t));
    }
    MphCtx* ctx = nullptr;
    if (nslabs > 1) {
        // one slab rank: every rank reads the same files and keeps the particles of its slab
        MphSlabOptions o{};
        o.rank = R.rank;
        o.nranks = nslabs;
        o.axis = std::getenv("MPH_SLAB_AXIS") ? std::atoi(std::getenv("MPH_SLAB_AXIS")) : (cfg.dim == 3 ? 2 : 0);
        char uid[128] = {0};
        if (host_transport) {
            o.host_fn = socket_exchange;
            o.host_user = &R;
        } else {
            if (root) {
                rc = mph_dist_unique_id(uid);
                if (rc) die(nullptr, rc, "mph_dist_unique_id");
                for (int fd : R.uid_out)
                    if (!write_all(fd, uid, sizeof(uid))) die(nullptr, MPH_ERR_TRANSPORT, "handing out the RCCL id");
            } else if (!read_all(R.uid_fd, uid, sizeof(uid))) {
                die(nullptr, MPH_ERR_TRANSPORT, "receiving the RCCL id");
            }
            o.unique_id128 = uid;
        }
        if (!(std::getenv("MPH_SLAB_SHARE_DEVICE") && std::atoi(std::getenv("MPH_SLAB_SHARE_DEVICE")))) {
            int ndev = 0;
            if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) device = (device + R.rank) % ndev;
        }
        rc = mph_create_slab(&ctx, &cfg, n, prop.data(), pos.data(), pos0.data(), vel.data(), device, &o);
        if (rc) die(ctx, rc, "mph_create_slab");
    } else {
        rc = mph_create(&ctx, &cfg, n, prop.data(), pos.data(), pos0.data(), vel.data(), device);
        if (rc) die(ctx, rc, "mph_create");
    }
    double sc[36];
    mph_get_scalars(ctx, sc);
    logf("N0a = %e\nN0p = %e\n", sc[0], sc[1]);
    rc = mph_write_vtk(ctx, "output.vtk");
    if (rc) die(ctx, rc, "writing output.vtk");
    {
        time_t t = time(nullptr);
        logf("start main roop at %s\n", ctime(&t));
    }
    // the reference's timing buckets (main.cpp:695-700) from HIP events, opt-in (single GPU,
    // MPH_PHASE_TIMING=1): with them on, mph_step launches every step's kernels directly instead of
    // replaying the captured graphs (HIP cannot time events inside a graph) and waits for the
    // events after every batch of up to 8 steps
    const bool phases = nslabs == 1 && std::getenv("MPH_PHASE_TIMING") && std::atoi(std::getenv("MPH_PHASE_TIMING")) == 1;
    if (phases) {
        rc = mph_phase_timing(ctx, 1);
        if (rc) die(ctx, rc, "mph_phase_timing");
    }
    const double dt = cfg.dt;
    // MPH_DIST_MONITOR=<csv path> with MPH_SLABS > 1: the same file from the slab ranks' records
    // (include/mph_gpu.h mph_dist_monitor_*) -- every rank configures and makes the collective read
    // where a single context reads its ring, rank 0 receives the combined samples and writes them
    MonitorCsv mon;
    const bool dmon = nslabs > 1 && std::getenv("MPH_DIST_MONITOR");
    if (const char* mp = std::getenv(dmon ? "MPH_DIST_MONITOR" : "MPH_MONITOR")) {
        if (const char* e = std::getenv("MPH_MONITOR_STRIDE")) mon.stride = std::atoi(e);
        for (double v : parse_numbers(std::getenv("MPH_MONITOR_TRACK"))) mon.track.push_back((int)v);
        mon.probes = parse_numbers(std::getenv("MPH_MONITOR_PROBES"));
        if (mon.probes.size() % 3 != 0) die(nullptr, MPH_ERR_ARG, "MPH_MONITOR_PROBES (x,y,z;x,y,z;...)");
        // free-surface gauges beside the monitors (include/mph_gpu.h mph_gauge_configure): lines
        // through these points along MPH_MONITOR_GAUGE_AXIS (default -1: gravity's) of radius
        // MPH_MONITOR_GAUGE_RADIUS (default 0: RadiusRatioP dx)
        mon.gauges = parse_numbers(std::getenv("MPH_MONITOR_GAUGES"));
        if (mon.gauges.size() % 3 != 0) die(nullptr, MPH_ERR_ARG, "MPH_MONITOR_GAUGES (x,y,z;x,y,z;...)");
        if (dmon && !mon.gauges.empty())
            die(nullptr, MPH_ERR_UNSUPPORTED, "MPH_MONITOR_GAUGES with MPH_DIST_MONITOR (gauges need a single context)");
        // the ring holds the samples of the longest batch the loop below issues: a batch ends at the
        // next .prof or .vtk output step or at EndTime
        const double span = std::fmin(std::fmin(cfg.output_interval, cfg.vtk_output_interval), cfg.end_time - cfg.time);
        const double most = std::fmin(std::fmax(span, 0.0) / dt + 4.0, 1.0e8);
        MphMonitorConfig mc{};
        mc.stride = mon.stride;
        mc.capacity = (int)(most / (mon.stride > 0 ? mon.stride : 1)) + 2;
        mc.ntrack = (int)mon.track.size();
        mc.track = mon.track.data();
        mc.nprobe = (int)(mon.probes.size() / 3);
        mc.probes = mon.probes.data();
        rc = dmon ? mph_dist_monitor_configure(ctx, &mc) : mph_monitor_configure(ctx, &mc);
        if (rc) die(ctx, rc, dmon ? "mph_dist_monitor_configure" : "mph_monitor_configure");
        if (!mon.gauges.empty()) {
            MphGaugeConfig gc{};
            gc.axis = std::getenv("MPH_MONITOR_GAUGE_AXIS") ? std::atoi(std::getenv("MPH_MONITOR_GAUGE_AXIS")) : -1;
            gc.ngauge = (int)(mon.gauges.size() / 3);
            gc.points = mon.gauges.data();
            gc.radius = std::getenv("MPH_MONITOR_GAUGE_RADIUS") ? std::atof(std::getenv("MPH_MONITOR_GAUGE_RADIUS")) : 0.0;
            rc = mph_gauge_configure(ctx, &gc);
            if (rc) die(ctx, rc, "mph_gauge_configure");
        }
        mon.width = dmon ? MPH_MONITOR_HEAD + 6 * mc.ntrack + 2 * mc.nprobe : mph_monitor_sample_doubles(ctx);
        mon.buf.resize((size_t)mc.capacity * mon.width);
        if (root) {
            mon.f = std::fopen(mp, "w");
            if (!mon.f) die(nullptr, MPH_ERR_IO, "opening the MPH_MONITOR file");
            monitor_header(mon);
        }
    }
    // MPH_SAMPLE="ox,oy,oz;sx,sy,sz;nx,ny,nz": at every VTK output step the fields are sampled on
    // that lattice (include/mph_gpu.h mph_sample_grid; MPH_SAMPLE_RADIUS, MPH_SAMPLE_CLASSES
    // optional) and written as VTK ImageData to MPH_SAMPLE_FILE, a printf pattern taking the .vtk
    // files' index (default sample%03d.vti).  MPH_DIST_SAMPLE with MPH_SLABS > 1: the same grammar,
    // options, file and cadence from the slab ranks (include/mph_gpu.h mph_dist_sample_grid) -- every
    // rank samples the lattice planes it owns, rank 0 receives the lattice and writes the file
    MphSampleGrid sgrid{};
    std::vector<double> sbuf;
    std::string sfile = "sample%03d.vti";
    const bool dsample = nslabs > 1 && std::getenv("MPH_DIST_SAMPLE");
    const bool sampling = dsample || std::getenv("MPH_SAMPLE") != nullptr;
    if (sampling) {
        const std::vector<double> v = parse_numbers(std::getenv(dsample ? "MPH_DIST_SAMPLE" : "MPH_SAMPLE"));
        if (v.size() != 9) die(nullptr, MPH_ERR_ARG, "MPH_SAMPLE / MPH_DIST_SAMPLE (ox,oy,oz;sx,sy,sz;nx,ny,nz)");
        double points = 1.0;
        for (int d = 0; d < 3; ++d) {
            sgrid.origin[d] = v[d];
            sgrid.spacing[d] = v[3 + d];
            if (!(v[6 + d] >= 1.0 && v[6 + d] <= MPH_SAMPLE_MAX_POINTS)) die(nullptr, MPH_ERR_ARG, "MPH_SAMPLE counts");
            sgrid.count[d] = (int)v[6 + d];
            points *= sgrid.count[d];
        }
        if (points > MPH_SAMPLE_MAX_POINTS) die(nullptr, MPH_ERR_ARG, "MPH_SAMPLE (too many points)");
        if (const char* e = std::getenv("MPH_SAMPLE_RADIUS")) sgrid.radius = std::atof(e);
        if (const char* e = std::getenv("MPH_SAMPLE_CLASSES")) sgrid.classes = std::atoi(e);
        if (const char* e = std::getenv("MPH_SAMPLE_FILE")) sfile = e;
        if (!dsample || root) sbuf.resize((size_t)points * MPH_SAMPLE_CHANNELS);
    }
    // MPH_OUTPUT_SELECT=<spec> (include/mph_gpu.h mph_selection_parse): every VTK-step file, .vtk or
    // .vtu, holds only that selection, evaluated at that step (written before the loop goes on: the
    // background writer takes whole frames only); the .prof restart files stay whole.
    // MPH_DIST_OUTPUT_SELECT with MPH_SLABS > 1: the same grammar and files from the slab ranks
    // (include/mph_gpu.h mph_dist_select, mph_dist_write_vtk_selected) -- every rank selects among the
    // particles it owns at that step and sends its selected rows, rank 0 merges them and writes the
    // file; the .prof files and output.vtk stay whole.
    MphSelection out_sel{};
    const bool dout_select = nslabs > 1 && std::getenv("MPH_DIST_OUTPUT_SELECT");
    const bool out_select = dout_select || std::getenv("MPH_OUTPUT_SELECT") != nullptr;
    if (out_select && mph_selection_parse(std::getenv(dout_select ? "MPH_DIST_OUTPUT_SELECT" : "MPH_OUTPUT_SELECT"), &out_sel) != MPH_OK)
        die(nullptr, MPH_ERR_ARG, "MPH_OUTPUT_SELECT / MPH_DIST_OUTPUT_SELECT "
                                  "(types=..;box=x0,y0,z0,x1,y1,z1;on=position|initial;every=..;phase=..)");
    // MPH_KINEMATICS="radius=..;classes=..;beta=..;det=.." (include/mph_gpu.h mph_kinematics_parse; any
    // subset of the keys, empty text: the defaults): at every VTK output step the velocity gradient,
    // vorticity and free-surface fields are computed (mph_compute_kinematics) and written as a .vtu to
    // MPH_KINEMATICS_FILE, a printf pattern taking the .vtk files' index (default kin%03d.vtu), cropped
    // to MPH_OUTPUT_SELECT where that is set
    MphKinematics kin{};
    std::string kfile = "kin%03d.vtu";
    const bool kinematics = std::getenv("MPH_KINEMATICS") != nullptr;
    if (kinematics) {
        if (mph_kinematics_parse(std::getenv("MPH_KINEMATICS"), &kin) != MPH_OK)
            die(nullptr, MPH_ERR_ARG, "MPH_KINEMATICS (radius=..;classes=..;beta=..;det=..)");
        if (const char* e = std::getenv("MPH_KINEMATICS_FILE")) kfile = e;
    }
    // MPH_LOADS=<csv path>: every MPH_LOADS_STRIDE-th step (default 10) of this run the selection
    // MPH_LOADS_SELECT (default: every particle) is made and one row appended: step (counted from the
    // start of the run), time, and the MPH_TOTALS totals about MPH_LOADS_CENTER=x,y,z (default the
    // origin) as %.17g -- the summed Force and its torque among them.  Force is stored by the last
    // step of an mph_step call, so the loop below ends its call on every such step: a loads row is a
    // flush point (DESIGN.md section 13 has its cost).
    // MPH_DIST_LOADS=<csv path> with MPH_SLABS > 1: the same options, header, rows and cadence from the
    // slab ranks (include/mph_gpu.h mph_dist_select, mph_dist_selection_totals) -- every rank reduces
    // its own selection, rank 0 combines the records in rank order and writes the row.  A slab step
    // stores Force on every step, but a row is evaluated on the state at its step, so the call ends
    // there all the same.
    const bool dloads = nslabs > 1 && std::getenv("MPH_DIST_LOADS");
    bool loads_on = false;
    FILE* loads_f = nullptr;
    MphSelection loads_sel{};
    loads_sel.every = 1;
    int loads_stride = 10;
    double loads_center[3] = {0.0, 0.0, 0.0};
    if (const char* lp = std::getenv(dloads ? "MPH_DIST_LOADS" : "MPH_LOADS")) {
        loads_on = true;
        if (const char* e = std::getenv("MPH_LOADS_SELECT"))
            if (mph_selection_parse(e, &loads_sel) != MPH_OK) die(nullptr, MPH_ERR_ARG, "MPH_LOADS_SELECT (a selection spec)");
        if (const char* e = std::getenv("MPH_LOADS_STRIDE")) loads_stride = std::atoi(e);
        if (loads_stride < 1) die(nullptr, MPH_ERR_ARG, "MPH_LOADS_STRIDE (>= 1)");
        if (const char* e = std::getenv("MPH_LOADS_CENTER")) {
            const std::vector<double> v = parse_numbers(e);
            if (v.size() != 3) die(nullptr, MPH_ERR_ARG, "MPH_LOADS_CENTER (x,y,z)");
            for (int d = 0; d < 3; ++d) loads_center[d] = v[d];
        }
        if (root) loads_f = std::fopen(lp, "w");
        if (root && !loads_f) die(nullptr, MPH_ERR_IO, "opening the MPH_LOADS file");
        static const char* cols[MPH_TOTALS] = {"count", "mass", "px", "py", "pz", "ke", "fx", "fy", "fz", "tx", "ty", "tz",
                                               "mx", "my", "mz", "xmin", "xmax", "ymin", "ymax", "zmin", "zmax", "vmax2",
                                               "reserved0", "reserved1"};
        if (loads_f) {
            std::fprintf(loads_f, "step,time");
            for (int k = 0; k < MPH_TOTALS; ++k) std::fprintf(loads_f, ",%s", cols[k]);
            std::fprintf(loads_f, "\n");
        }
    }
    const auto loop_t0 = std::chrono::steady_clock::now();
    double time_now = cfg.time;
    int istep = (int)(time_now / dt);
    double out_next = 0.0, vtk_next = 0.0;
    const bool vtu = vtk.size() > 4 && vtk.compare(vtk.size() - 4, 4, ".vtu") == 0;
    long long steps_run = 0;
    double loop_s = 0.0;
    char name[1024];
    while (time_now < cfg.end_time + 1.0e-5 * dt) {
        if (time_now + 1.0e-5 * dt >= out_next) {
            std::snprintf(name, sizeof(name), prof.c_str(), istep);
            roctxRangePushA("write_prof");
            rc = mph_write_prof(ctx, name);
            roctxRangePop();
            if (rc) die(ctx, rc, "writing a .prof file");
            logf("@ Prof Output Time : %e\n", time_now);
            out_next += cfg.output_interval;
        }
        // run until the next step that produces output (same Time additions as the reference)
        int k = 0;
        double t = time_now;
        bool vtk_after = false;
        while (t < cfg.end_time + 1.0e-5 * dt) {
            ++k;
            if (t + 1.0e-5 * dt >= vtk_next) { vtk_after = true; break; }
            t += dt;
            if (t + 1.0e-5 * dt >= out_next || !(t < cfg.end_time + 1.0e-5 * dt)) break;
            if (loads_on && (steps_run + k) % loads_stride == 0) break;   // (that step stores Force)
        }
        const bool loads_after = loads_on && (steps_run + k) % loads_stride == 0;
        const auto t0 = std::chrono::steady_clock::now();
        roctxRangePushA("mph_step");
        rc = mph_step(ctx, k);
        if (rc) die(ctx, rc, "mph_step");
        mph_synchronize(ctx);
        roctxRangePop();
        if (mon.width) {
            long long lost = 0;
            const long long most = (long long)(mon.buf.size() / mon.width);
            const long long got = dmon ? mph_dist_monitor_read(ctx, mon.buf.data(), most, &lost)
                                       : mph_monitor_read(ctx, mon.buf.data(), most, &lost);
            if (got < 0) die(ctx, (int)got, dmon ? "mph_dist_monitor_read" : "mph_monitor_read");
            if (lost) logf("error: the monitor ring overwrote %lld unread samples (ring sized too small)\n", lost);
            for (long long r = 0; r < got; ++r) {
                for (int k = 0; k < mon.width; ++k)
                    std::fprintf(mon.f, k ? ",%.17g" : "%.17g", mon.buf[(size_t)r * mon.width + k]);
                std::fprintf(mon.f, "\n");
            }
            if (mon.f) std::fflush(mon.f);
        }
        // fault injection for the failure-propagation test (tests/test_gpu_driver.py): this rank
        // fails after its first batch
        if (const char* f = std::getenv("MPH_FAIL_RANK"))
            if (nslabs > 1 && std::atoi(f) == R.rank) die(ctx, MPH_ERR_ARG, "MPH_FAIL_RANK fault injection");
        loop_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        steps_run += k;
        if (loads_after) {
            double tot[MPH_TOTALS];
            rc = dloads ? mph_dist_select(ctx, &loads_sel, nullptr) : mph_select(ctx, &loads_sel, nullptr);
            if (rc) die(ctx, rc, dloads ? "mph_dist_select (MPH_LOADS_SELECT)" : "mph_select (MPH_LOADS_SELECT)");
            rc = dloads ? mph_dist_selection_totals(ctx, loads_center, tot) : mph_selection_totals(ctx, loads_center, tot);
            if (rc) die(ctx, rc, dloads ? "mph_dist_selection_totals" : "mph_selection_totals");
            if (loads_f) {
                std::fprintf(loads_f, "%lld,%.17g", steps_run, mph_time(ctx));
                for (int q = 0; q < MPH_TOTALS; ++q) std::fprintf(loads_f, ",%.17g", tot[q]);
                std::fprintf(loads_f, "\n");
                std::fflush(loads_f);
            }
        }
        for (int s = 0; s < k; ++s) {
            if (vtk_after && s == k - 1 && sampling) {
                rc = dsample ? mph_dist_sample_grid(ctx, &sgrid, sbuf.empty() ? nullptr : sbuf.data())
                             : mph_sample_grid(ctx, &sgrid, sbuf.data());
                if (rc) die(ctx, rc, dsample ? "mph_dist_sample_grid" : "mph_sample_grid");
                std::snprintf(name, sizeof(name), sfile.c_str(), istep);
                if (!dsample || root) {
                    rc = mph_write_vti_arrays(name, &sgrid, sbuf.data());
                    if (rc) die(ctx, rc, "writing a .vti file");
                }
            }
            if (vtk_after && s == k - 1 && kinematics) {
                rc = mph_compute_kinematics(ctx, &kin);
                if (rc) die(ctx, rc, "mph_compute_kinematics");
                std::snprintf(name, sizeof(name), kfile.c_str(), istep);
                if (out_select) {
                    rc = mph_select(ctx, &out_sel, nullptr);
                    if (rc) die(ctx, rc, "mph_select (MPH_OUTPUT_SELECT)");
                    rc = mph_write_vtu_kinematics_selected(ctx, name);
                } else {
                    rc = mph_write_vtu_kinematics(ctx, name);
                }
                if (rc) die(ctx, rc, "writing a kinematics .vtu file");
            }
            if (vtk_after && s == k - 1) {
                // main.cpp:672-673: the virial diagnostic runs before every VTK write
                roctxRangePushA("virial");
                rc = mph_compute_virial(ctx);
                roctxRangePop();
                if (rc) die(ctx, rc, "mph_compute_virial");
                std::snprintf(name, sizeof(name), vtk.c_str(), istep);
                // formatted and written by a background thread while the next steps run
                if (dout_select) {
                    rc = mph_dist_select(ctx, &out_sel, nullptr);
                    if (rc) die(ctx, rc, "mph_dist_select (MPH_DIST_OUTPUT_SELECT)");
                    rc = vtu ? mph_dist_write_vtu_selected(ctx, name) : mph_dist_write_vtk_selected(ctx, name);
                } else if (out_select) {
                    rc = mph_select(ctx, &out_sel, nullptr);
                    if (rc) die(ctx, rc, "mph_select (MPH_OUTPUT_SELECT)");
                    rc = vtu ? mph_write_vtu_selected(ctx, name) : mph_write_vtk_selected(ctx, name);
                } else {
                    rc = vtu ? mph_write_vtu(ctx, name) : mph_write_vtk_async(ctx, name);
                }
                if (rc) die(ctx, rc, "writing a .vtk file");
                logf("@ Vtk Output Time : %e\n", time_now);
                vtk_next += cfg.vtk_output_interval;
            }
            time_now += dt;
            istep++;
        }
    }
    {
        const double total_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - loop_t0).count();
        time_t t = time(nullptr);
        logf("end main roop at %s\n", ctime(&t));
        if (phases) {
            // main.cpp:695-700, in GPU seconds from HIP events; "other" is the rest of the loop's
            // wall time (file output, host work, launch gaps)
            double ph[3] = {0.0, 0.0, 0.0};
            mph_phase_times(ctx, ph);
            const double nb = ph[0] * 1e-3, ex = ph[1] * 1e-3, vi = ph[2] * 1e-3;
            const double other = total_s - nb - ex - vi;
            logf("neighbor search:         %lf [GPU sec]\n", nb);
            logf("explicit calculation:    %lf [GPU sec]\n", ex);
            logf("virial calculation:      %lf [GPU sec]\n", vi);
            logf("other calculation:       %lf [sec]\n", other);
            logf("total:                   %lf [sec]\n", nb + ex + vi + other);
            logf("total (check):           %lf [sec]\n", total_s);
        }
        logf("step loop (wall):        %lf [sec] for %lld steps\n", loop_s, steps_run);
        if (loop_s > 0)
            logf("throughput:              %e [particle-steps/sec]\n", (double)n * steps_run / loop_s);
    }
    rc = mph_output_wait(ctx);
    if (rc) die(ctx, rc, "writing a .vtk file");
    mph_destroy(ctx);
    if (mon.f) std::fclose(mon.f);
    if (loads_f) std::fclose(loads_f);
    if (g_log) std::fclose(g_log);
    // rank 0 waits for the other ranks (the SIGCHLD handler reaps them and ends the run if one failed)
    for (;;) {
        bool running = false;
        for (int k = 0; k < g_nchildren; ++k) running = running || g_child_done[k] == 0;
        if (!running) break;
        usleep(1000);
    }
    return 0;
}
