// fh_pool.hip — ONE batch over several GPUs of a node, behind the C ABI (include/fasterhip.h, fh_pool_*).
//
// every genNewTraj() is independent and a whole+safe pair never leaves its GPU, so a batch is cut into
// contiguous blocks (device g solves problems [g*ceil(n/G), (g+1)*ceil(n/G)) — the same rule as faster_amd/shard.py), every
// device gets its block straight from the caller's host arrays (asynchronous H2D on the device's own stream: a scatter needs
// no collective), solves it with the single-device entry points, and the complete fh_result blocks come back either to the
// caller's host array or, for a device-resident consumer, into ONE device's memory with peer copies over xGMI
// (hipMemcpyPeerAsync; the all-to-one "gather" of the batch).  One host thread per device drives its stream, so the copies
// and solves of the devices overlap even from pageable host memory.  There is no CPU fallback: no device, no pool.
//
// The one-process-per-GPU form of the same thing (torch.distributed, RCCL all_gather of the result blocks) is bench.py
// --scaling strong; both use the block partition, so results are identical to the 1-way run by construction
// (tests/test_distributed_gloo.py, tests/test_gpu_parity.py::test_pool_shards_equal_one_way).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fasterhip.h"
#include "fh_host.hpp"

namespace {

struct PoolDev {
  int device = -1;
  fh_ctx* ctx = nullptr;
  hipStream_t stream = nullptr;
  // this device's block of a job (no launch is in flight between two jobs: run_shard ends in fh_sync), and the unknown voxel flags
  // (fh_pool_set_unknown_grid), which the context's launches read until they are set again
  enum Buf { PROBLEMS, FACES, RESULTS, SAFE_PROBLEMS, SAFE_FACES, SAFE_RESULTS, UNKNOWN_FLAGS, N_BUFS };
  fhh::DeviceBuffer buf[N_BUFS];
  std::string err;
  int rc = FH_OK;
};

}  // namespace

struct fh_pool {
  std::vector<PoolDev> dev;
  std::string err;
};

namespace {

#define POOL_HIP(call) FHH_HIP(call, d.err, d.rc = FH_ERR_DEVICE; return)

// contiguous block partition (pairs are never split): the rule of faster_amd/shard.py::shard_range
void shard_range(int n, int g, int G, int& lo, int& hi) {
  const int per = (n + G - 1) / G;
  lo = std::min(g * per, n);
  hi = std::min(lo + per, n);
}

struct Job {
  const fh_problem* problems;
  const fh_face* faces;
  int64_t n_faces;
  int n;
  fh_result* results;        // host array of n records, or null
  fh_result* d_results_root; // device array of n records on dev[root], or null
  int root;
  // pairs
  bool pairs;
  const fh_problem* safe_templates;
  double r_frac, shrink;
  int max_safe_poly;
  fh_result* safe_results;
  fh_result* d_safe_results_root;
};

void run_shard(fh_pool* pool, int g, const Job& job) {
  PoolDev& d = pool->dev[(size_t)g];
  d.rc = FH_OK;
  d.err.clear();
  int lo, hi;
  shard_range(job.n, g, (int)pool->dev.size(), lo, hi);
  const int m = hi - lo;
  if (m <= 0) return;
  POOL_HIP(hipSetDevice(d.device));
  // this shard's rows of the face array, and its problems rebased onto them
  std::vector<fh_problem> pr(job.problems + lo, job.problems + hi);
  const fhh::BatchScan scan = fhh::scan_batch(pr.data(), m, job.n_faces);
  if (scan.first_outside >= 0) {
    d.err = "fh_pool: a problem addresses faces outside [0, n_faces)";
    d.rc = FH_ERR_ARG;
    return;
  }
  const int64_t f_lo = scan.face_lo, f_hi = scan.face_hi;
  for (fh_problem& p : pr)
    if (p.n_poly >= 1 && p.n_poly <= FH_MAX_POLY && p.face_begin >= f_lo) p.face_begin -= (int32_t)f_lo;
  const size_t pb = sizeof(fh_problem) * (size_t)m, fb = sizeof(fh_face) * (size_t)std::max<int64_t>(f_hi - f_lo, 1), rb = sizeof(fh_result) * (size_t)m;
  const size_t need[6] = {pb, fb, rb, pb, fb, rb};  // (in the order of PoolDev::Buf; the safe three for pairs only)
  for (int b = 0; b < (job.pairs ? 6 : 3); b++)
    if (d.buf[b].reserve(need[b], d.stream) != hipSuccess) {
      d.err = "fh_pool: out of device memory";
      d.rc = FH_ERR_NOMEM;
      return;
    }
  fh_problem *d_problems = d.buf[PoolDev::PROBLEMS].as<fh_problem>(), *d_safe = d.buf[PoolDev::SAFE_PROBLEMS].as<fh_problem>();
  fh_face *d_faces = d.buf[PoolDev::FACES].as<fh_face>(), *d_safe_faces = d.buf[PoolDev::SAFE_FACES].as<fh_face>();
  fh_result *d_results = d.buf[PoolDev::RESULTS].as<fh_result>(), *d_safe_results = d.buf[PoolDev::SAFE_RESULTS].as<fh_result>();
  POOL_HIP(hipMemcpyAsync(d_problems, pr.data(), pb, hipMemcpyHostToDevice, d.stream));
  if (f_hi > f_lo) POOL_HIP(hipMemcpyAsync(d_faces, job.faces + f_lo, sizeof(fh_face) * (size_t)(f_hi - f_lo), hipMemcpyHostToDevice, d.stream));
  int rc;
  if (job.pairs) {
    POOL_HIP(hipMemcpyAsync(d_safe, job.safe_templates + lo, pb, hipMemcpyHostToDevice, d.stream));
    rc = fh_solve_pairs_device(d.ctx, d_problems, d_faces, m, scan.max_seg, scan.max_faces, job.r_frac, job.shrink, job.max_safe_poly, d_results,
                               d_safe, d_safe_faces, d_safe_results);
  } else {
    rc = fh_solve_batch_device(d.ctx, d_problems, d_faces, m, scan.max_seg, scan.max_faces, d_results);
  }
  if (rc != FH_OK) {
    d.err = fh_last_error(d.ctx);
    d.rc = rc;
    return;
  }
  // the gather: complete fh_result blocks to the host array, or into the root device's memory over xGMI
  if (job.results) POOL_HIP(hipMemcpyAsync(job.results + lo, d_results, rb, hipMemcpyDeviceToHost, d.stream));
  if (job.pairs && job.safe_results) POOL_HIP(hipMemcpyAsync(job.safe_results + lo, d_safe_results, rb, hipMemcpyDeviceToHost, d.stream));
  if (job.d_results_root) {
    const int root_dev = pool->dev[(size_t)job.root].device;
    POOL_HIP(hipMemcpyPeerAsync(job.d_results_root + lo, root_dev, d_results, d.device, rb, d.stream));
    if (job.pairs && job.d_safe_results_root)
      POOL_HIP(hipMemcpyPeerAsync(job.d_safe_results_root + lo, root_dev, d_safe_results, d.device, rb, d.stream));
  }
  rc = fh_sync(d.ctx);
  if (rc != FH_OK) {
    d.err = fh_last_error(d.ctx);
    d.rc = rc;
  }
}

int run_job(fh_pool* pool, const Job& job) {
  if (job.n == 0) return FH_OK;
  fhh::DeviceScope restore(pool->dev[0].device);  // (run_shard makes its device current: the caller's comes back when the job is over)
  std::vector<std::thread> threads;
  const int G = (int)pool->dev.size();
  for (int g = 1; g < G; g++) threads.emplace_back(run_shard, pool, g, std::cref(job));
  run_shard(pool, 0, job);
  for (std::thread& t : threads) t.join();
  for (const PoolDev& d : pool->dev)
    if (d.rc != FH_OK) {
      pool->err = "device " + std::to_string(d.device) + ": " + d.err;
      return d.rc;
    }
  return FH_OK;
}

}  // namespace

extern "C" {

int fh_pool_create(fh_pool** out, const int* devices, int n_devices) {
  if (!out) return FH_ERR_ARG;
  *out = nullptr;
  fh_pool* pool = new (std::nothrow) fh_pool();
  if (!pool) return FH_ERR_NOMEM;
  *out = pool;
  int count = 0;
  const hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    pool->err = std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    return FH_ERR_DEVICE;
  }
  if (n_devices <= 0) n_devices = count;
  for (int g = 0; g < n_devices; g++) {
    PoolDev d;
    d.device = devices ? devices[g] : g;
    if (d.device < 0 || d.device >= count) {
      pool->err = "fh_pool_create: device index out of range";
      return FH_ERR_ARG;
    }
    fhh::DeviceScope scope(d.device);
    if (!scope.ok || hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking) != hipSuccess) {
      pool->err = "fh_pool_create: cannot create a stream on device " + std::to_string(d.device);
      return FH_ERR_DEVICE;
    }
    const int rc = fh_create(&d.ctx, d.device);
    if (rc != FH_OK) {
      pool->err = d.ctx ? fh_last_error(d.ctx) : "fh_create failed";
      if (d.ctx) fh_destroy(d.ctx);
      return rc;
    }
    (void)fh_set_stream(d.ctx, d.stream);
    pool->dev.push_back(d);
  }
  // peer access for the device-resident gather (ignored where the pair of devices does not support it: the copy then stages)
  for (const PoolDev& a : pool->dev)
    for (const PoolDev& b : pool->dev)
      if (a.device != b.device) {
        int can = 0;
        fhh::DeviceScope scope(a.device);
        if (hipDeviceCanAccessPeer(&can, a.device, b.device) == hipSuccess && can && scope.ok) (void)hipDeviceEnablePeerAccess(b.device, 0);
      }
  (void)hipGetLastError();
  return FH_OK;
}

void fh_pool_destroy(fh_pool* pool) {
  if (!pool) return;
  for (PoolDev& d : pool->dev) {
    fhh::DeviceScope scope(d.device);
    if (d.ctx) fh_destroy(d.ctx);
    for (fhh::DeviceBuffer& b : d.buf) b.release();
    if (d.stream) (void)hipStreamDestroy(d.stream);
  }
  delete pool;
}

int fh_pool_size(const fh_pool* pool) { return pool ? (int)pool->dev.size() : 0; }
const char* fh_pool_last_error(const fh_pool* pool) { return pool ? pool->err.c_str() : "null pool"; }

int fh_pool_set_params(fh_pool* pool, const fh_params* p) {
  if (!pool || !p) return FH_ERR_ARG;
  for (PoolDev& d : pool->dev) {
    const int rc = fh_set_params(d.ctx, p);
    if (rc != FH_OK) return rc;
  }
  return FH_OK;
}

int fh_pool_set_pair_margin(fh_pool* pool, double r_margin) {
  if (!pool) return FH_ERR_ARG;
  for (PoolDev& d : pool->dev) {
    const int rc = fh_set_pair_margin(d.ctx, r_margin);
    if (rc != FH_OK) return rc;
  }
  return FH_OK;
}

int fh_pool_set_pair_rule(fh_pool* pool, const fh_pair_rule* rule) {
  if (!pool || !rule) return FH_ERR_ARG;
  for (PoolDev& d : pool->dev) {
    const int rc = fh_set_pair_rule(d.ctx, rule);
    if (rc != FH_OK) return rc;
  }
  return FH_OK;
}

// Unknown space as an input for the pool (rule mode 2): the flags are host memory here — every device of the pool gets its own copy
// (synchronous) and its context is told (fh_set_unknown_grid_device).  flags = NULL: none.
int fh_pool_set_unknown_grid(fh_pool* pool, const fh_voxel_grid* grid, const unsigned char* flags) {
  if (!pool) return FH_ERR_ARG;
  if (flags && !fhh::voxel_grid_ok(grid, false)) return FH_ERR_ARG;  // (the cell size: fh_set_unknown_grid_device)
  for (PoolDev& d : pool->dev) {
    fhh::DeviceScope scope(d.device);
    int rc = FH_OK;
    if (!flags) {
      rc = fh_set_unknown_grid_device(d.ctx, nullptr, nullptr);
    } else {
      const size_t bytes = (size_t)fhh::voxel_grid_cells(*grid);
      fhh::DeviceBuffer& d_flags = d.buf[PoolDev::UNKNOWN_FLAGS];
      // the context must not keep pointing at a buffer that reserve() may free: no launch of it is running (fh_sync waits for the CONTEXT's
      // stream, whichever it is), it forgets the old flags first, and learns the new ones only once they are in place
      (void)fh_sync(d.ctx);
      (void)hipStreamSynchronize(d.stream);
      (void)fh_set_unknown_grid_device(d.ctx, nullptr, nullptr);
      if (d_flags.reserve(bytes, d.stream) != hipSuccess || hipMemcpy(d_flags.ptr, flags, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = FH_ERR_DEVICE;
      else rc = fh_set_unknown_grid_device(d.ctx, grid, d_flags.as<const unsigned char>());
    }
    if (rc != FH_OK) {
      pool->err = "fh_pool_set_unknown_grid: device " + std::to_string(d.device);
      return rc;
    }
  }
  return FH_OK;
}

int fh_pool_solve_batch(fh_pool* pool, const fh_problem* problems, const fh_face* faces, int64_t n_faces, int n, fh_result* results,
                        int root, fh_result* d_results_root) {
  if (!pool || n < 0 || n_faces < 0) return FH_ERR_ARG;
  if (pool->dev.empty()) return FH_ERR_DEVICE;
  if (n == 0) return FH_OK;
  if (!problems || (!results && !d_results_root) || (n_faces > 0 && !faces)) return FH_ERR_ARG;
  if (d_results_root && (root < 0 || root >= (int)pool->dev.size())) return FH_ERR_ARG;
  Job job;
  std::memset(&job, 0, sizeof(job));
  job.problems = problems; job.faces = faces; job.n_faces = n_faces; job.n = n; job.results = results;
  job.d_results_root = d_results_root; job.root = root;
  return run_job(pool, job);
}

int fh_pool_solve_pairs(fh_pool* pool, const fh_problem* whole, const fh_face* faces, int64_t n_faces, int n,
                        const fh_problem* safe_templates, double r_frac, double shrink, int max_safe_poly, fh_result* whole_results,
                        fh_result* safe_results, int root, fh_result* d_whole_results_root, fh_result* d_safe_results_root) {
  if (!pool || n < 0 || n_faces < 0) return FH_ERR_ARG;
  if (pool->dev.empty()) return FH_ERR_DEVICE;
  if (n == 0) return FH_OK;
  if (!whole || !safe_templates || (n_faces > 0 && !faces)) return FH_ERR_ARG;
  if ((!whole_results || !safe_results) && (!d_whole_results_root || !d_safe_results_root)) return FH_ERR_ARG;
  if (d_whole_results_root && (root < 0 || root >= (int)pool->dev.size())) return FH_ERR_ARG;
  if (d_safe_results_root && !d_whole_results_root) return FH_ERR_ARG;  // (a device gather names both arrays or neither)
  Job job;
  std::memset(&job, 0, sizeof(job));
  job.problems = whole; job.faces = faces; job.n_faces = n_faces; job.n = n; job.results = whole_results;
  job.d_results_root = d_whole_results_root; job.root = root;
  job.pairs = true; job.safe_templates = safe_templates; job.r_frac = r_frac; job.shrink = shrink; job.max_safe_poly = max_safe_poly;
  job.safe_results = safe_results; job.d_safe_results_root = d_safe_results_root;
  return run_job(pool, job);
}

}  // extern "C"
