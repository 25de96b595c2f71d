// The host layer every .hip shares: HIP_TRY, launch and alignment arithmetic, the stage timers,
// the context object behind the opaque rs_ctx handle, and the layout of its scratch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "common.h"

namespace rs {
int hip_fail(hipError_t e, const char *what);  // "<what>: <hipGetErrorString>", RS_ENOMEM / RS_EDEVICE
}  // namespace rs

using rs::fail;
using rs::hip_fail;

#define HIP_TRY(expr)                                 \
  do {                                                \
    hipError_t e_ = (expr);                           \
    if (e_ != hipSuccess) return hip_fail(e_, #expr); \
  } while (0)

namespace rs {

constexpr size_t align256(size_t b) { return (b + 255) / 256 * 256; }

inline unsigned blocks(int64_t n, int per) { return static_cast<unsigned>((n + per - 1) / per); }

// HIP events around the kernels of a stage's next calls and the device ms between them: N events,
// created when first needed, and M slots that hold the last timed call's figures.  An untimed
// call (on == 0) does nothing here.
template <int N, int M>
struct StageTimer {
  int on = 0;
  hipEvent_t ev[N] = {};
  double ms[M];
  explicit StageTimer(double init) {
    for (double &v : ms) v = init;
  }
  // every event that is still missing is created, also after an earlier enable failed half way
  int enable(bool e) {
    if (e)
      for (hipEvent_t &x : ev)
        if (!x) HIP_TRY(hipEventCreate(&x));
    on = e ? 1 : 0;
    return RS_OK;
  }
  int mark(int k, hipStream_t s) {
    if (!on) return RS_OK;
    if (!ev[k]) HIP_TRY(hipEventCreate(&ev[k]));
    HIP_TRY(hipEventRecord(ev[k], s));
    return RS_OK;
  }
  // slot `slot` = (read) or += (add) the time between events a and b, once the stream that
  // recorded them has been waited for
  int read(int slot, int a, int b) { return elapsed(slot, a, b, false); }
  int add(int slot, int a, int b) { return elapsed(slot, a, b, true); }
  void copy_out(double *out) const {
    for (int k = 0; k < M; ++k) out[k] = ms[k];
  }
  void destroy() {
    for (hipEvent_t &x : ev) {
      if (x) (void)hipEventDestroy(x);
      x = nullptr;
    }
  }

 private:
  int elapsed(int slot, int a, int b, bool sum) {
    if (!on) return RS_OK;
    float t = 0.0f;
    HIP_TRY(hipEventElapsedTime(&t, ev[a], ev[b]));
    ms[slot] = sum ? ms[slot] + t : t;
    return RS_OK;
  }
};

}  // namespace rs

#define RS_BA_EVENTS 16  // one batch of rs_bundle_adjust kernels between two host waits

struct rs_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  // the parity parse's second stream (the second MT stream pass beside the entry kernel), one per
  // context, created with it: independent contexts never wait for each other's parse work
  hipStream_t aux_stream = nullptr;
  void *scratch = nullptr;     // grow-only device scratch for single-shot ops
  size_t scratch_bytes = 0;
  void *pinned = nullptr;      // grow-only pinned host staging of single-shot inputs (one DMA
  size_t pinned_bytes = 0;     // copy instead of several pageable ones; the ops synchronise)
  rs_f8_plan *np_plan = nullptr;  // cached plan of rs_f8_ransac_np
  rs_np_shard *np_shard = nullptr;  // world-1 parity-stream session (np_choice_device)
  void *comm = nullptr;        // ncclComm_t
  void *comm_buf = nullptr;    // device staging for collectives
  size_t comm_buf_bytes = 0;
  // rs_np_timing: HIP events between the parity-stream parse's steps (np_sampler.hip), the
  // last np_choice_device call's sums over its segments (RS_NP_TIMING_SLOTS ms, 3 byte counts)
  int np_timing = 0;
  double np_ms[RS_NP_TIMING_SLOTS] = {};
  double np_bytes[3] = {};
  int64_t np_segments = 0;
  // rs_pnp_timing: around the PnP-RANSAC solve and count kernels of the next calls (solve, count)
  rs::StageTimer<3, 2> pnp{-1.0};
  // rs_ba_timing: between the kernels of rs_bundle_adjust, the last timed call's sums per kernel
  // and its number of trials
  rs::StageTimer<RS_BA_EVENTS, RS_BA_TIMING_SLOTS> ba{0.0};
  int64_t ba_trials = 0;
  // rs_features_timing: around the kernels of the next front-end calls (features.hip), the last
  // timed call's device ms between its upload and its download
  rs::StageTimer<2, 1> feat{-1.0};
  // rs_tracking_timing: between the stages of the next rs_klt_track calls (tracking.hip):
  // pyramid, forward, backward
  rs::StageTimer<4, RS_TRACKING_TIMING_SLOTS> track{-1.0};
  // rs_cloud_timing: between the stages of the next point-cloud calls (cloud.hip), per stage
  rs::StageTimer<5, RS_CLOUD_TIMING_SLOTS> cloud{-1.0};
  // rs_cloud_knn_timing: between the stages of the next k-NN calls (cloud_knn.hip): box, grid,
  // scan, scatter, query, normals, mean_dist
  rs::StageTimer<8, RS_CLOUD_KNN_TIMING_SLOTS> knn{-1.0};
  // rs_surface_points_timing: between the stages of the next surface-from-points calls
  // (cloud_knn.hip): box, grid, scan, scatter, field
  rs::StageTimer<7, RS_SURFACE_POINTS_TIMING_SLOTS> points{-1.0};
  // rs_dense_timing: around the kernel of the next dense calls (dense.hip): plane sweep,
  // consistency
  rs::StageTimer<2, RS_DENSE_TIMING_SLOTS> dense{-1.0};
  // rs_dense_sgm_timing: between the stages of the next aggregation calls (dense_sgm.hip):
  // sweep, aggregate, select
  rs::StageTimer<4, RS_DENSE_SGM_TIMING_SLOTS> dense_sgm{-1.0};
  // rs_surface_timing: around the kernels of the next surface calls (surface.hip): integrate,
  // classify, scan, emit
  rs::StageTimer<5, RS_SURFACE_TIMING_SLOTS> surface{-1.0};
  // rs_surface_texture_timing: around the kernels of the next mesh-colouring calls
  // (surface_texture.hip): raster_small, raster_large, gather
  rs::StageTimer<4, RS_SURFACE_TEXTURE_TIMING_SLOTS> texture{-1.0};
  // rs_eval_timing: between the stages of the next mesh-distance calls (eval.hip): bin, scan,
  // scatter, query
  rs::StageTimer<5, RS_EVAL_TIMING_SLOTS> eval{-1.0};
  // rs_mesh_timing: around the kernels of the next mesh clean-up calls (mesh.hip): components,
  // compact, adjacency, smooth
  rs::StageTimer<3, RS_MESH_TIMING_SLOTS> mesh{-1.0};
  // rs_simplify_timing: between the stages of the next rs_mesh_simplify calls (simplify.hip):
  // cluster, rows, quadric, faces
  rs::StageTimer<5, RS_SIMPLIFY_TIMING_SLOTS> simplify{-1.0};
  // rs_global_timing: around the kernels of the next global-registration calls (global_reg.hip):
  // spfh, fpfh, match, solve, count, gather
  rs::StageTimer<9, RS_GLOBAL_TIMING_SLOTS> global{-1.0};
};

namespace rs {

int ensure_scratch(rs_ctx *c, size_t bytes);
int ensure_pinned(rs_ctx *c, size_t bytes);

// The buffers of one call, laid out in the order they are added: each starts where the one
// before it ended, its size padded to `pad` bytes (256, or 1 where a call packs its buffers), so
// a buffer of no elements takes no bytes and shares its offset with its successor.  The same
// offsets hold in the context's device scratch and in its pinned mirror.  The arithmetic needs
// no context; bind() gives the handles their pointers.
class Layout {
 public:
  template <class T>
  struct Buf {
    const Layout *in;
    size_t off, bytes;  // bytes: unpadded
    T *dev() const { return reinterpret_cast<T *>(in->d_ + off); }
    T *host() const { return reinterpret_cast<T *>(in->h_ + off); }
  };

  explicit Layout(size_t pad = 256) : pad_(pad) {}
  Layout(const Layout &) = delete;
  Layout &operator=(const Layout &) = delete;

  template <class T>
  Buf<T> add(size_t count) { return add_bytes<T>(sizeof(T) * count); }
  // a buffer sized in bytes: a T record with a tail of another type behind it
  template <class T>
  Buf<T> add_bytes(size_t bytes) {
    const Buf<T> b{this, total_, bytes};
    total_ += (bytes + pad_ - 1) / pad_ * pad_;
    return b;
  }
  // the next buffer starts at a multiple of m; returns the bytes skipped
  size_t skip_to(size_t m) {
    const size_t gap = (total_ + m - 1) / m * m - total_;
    total_ += gap;
    return gap;
  }
  size_t total() const { return total_; }
  // contiguous ranges for one copy: [start of the layout, start of x), [start of x, end of the
  // layout) and [start of a, start of b)
  template <class T>
  size_t upto(const Buf<T> &x) const { return x.off; }
  template <class T>
  size_t from(const Buf<T> &x) const { return total_ - x.off; }
  template <class A, class B>
  size_t span(const Buf<A> &a, const Buf<B> &b) const { return b.off - a.off; }

  void bind(void *dev, void *host) {
    d_ = static_cast<char *>(dev);
    h_ = static_cast<char *>(host);
  }
  // the context scratch grown to total() + slack and, where the call stages through pinned
  // memory, the pinned mirror grown to `pinned` bytes
  int bind(rs_ctx *c, size_t slack = 256, size_t pinned = 0) {
    int st = ensure_scratch(c, total_ + slack);
    if (!st && pinned) st = ensure_pinned(c, pinned);
    if (st) return st;
    bind(c->scratch, c->pinned);
    return RS_OK;
  }
  char *dev() const { return d_; }
  char *host() const { return h_; }

 private:
  size_t pad_, total_ = 0;
  char *d_ = nullptr, *h_ = nullptr;
};

// The size and index rules of the bundle-adjustment entry points (tables.hip).
int ba_check(int64_t nC, int64_t nP, const int32_t *ov, const int32_t *op, int64_t n);
void np_shard_free(rs_ctx *c);
int np_preload();  // the parse kernels' code object onto the current device (rs_ctx_create)
bool np_gpu_supported(int64_t n, int32_t k);  // within the GPU parse's population range
// The numpy (py: CPython) stream's next `count` choice(n, k) tuples; rows [skip, skip + take)
// (take < 0: to the end) are written to d_out (take * k int32); (key, pos) advance past all
// `count`.  Synchronous on the context stream.
int np_choice_enqueue(rs_ctx *c, const uint32_t *key, int32_t pos, int64_t n, int32_t k,
                      int64_t count, int32_t *d_out, bool *queued);
int np_choice_finish(rs_ctx *c, uint32_t *key, int32_t *pos, bool *rerun);
int np_choice_device(rs_ctx *c, uint32_t *key, int32_t *pos, int64_t n, int32_t k,
                     int64_t count, int32_t *d_out, bool py = false, int64_t skip = 0,
                     int64_t take = -1);
// Step 4 of a sharded parse (np_sampler.hip, rs_np_shard_*) into device memory.
int np_shard_tuples_device(rs_np_shard *w, int64_t base, int64_t hi, int64_t next_start,
                           int64_t final_idx, int32_t *d_out, uint32_t *key_out, int32_t *pos_out);
// The batched pair RANSAC (pairs.hip) enqueued without its download; the records (rs_pair_result
// layout), inlier lists and points stay on the device for the stages after it.
struct PairsDev {
  const void *pts;       // rsd::Pt per point (x1, y1, x2, y2), pair b at off[b]
  const int64_t *off;    // B + 1 offsets
  void *res;             // B records (rs_pair_result)
  int32_t *inl;          // S_RANSAC of pair b at inl[off[b] ..]
  int64_t total;         // off[B]
  char *extra;           // the caller's `extra` bytes of scratch (256-aligned)
};
int pairs_enqueue(rs_ctx *c, const double *p1, const double *p2, const int64_t *off, int64_t B,
                  int64_t H, int32_t mode, uint64_t seed_base, const int64_t *seed_ids,
                  const int32_t *host_tuples, double thresh, size_t extra, PairsDev *d);
// The plane sweep's argument rules (rs_dense_plane_sweep's RS_EINVAL list; `with_volume`: the
// D h w limit applies) and the launch of its kernel k_dense_sweep<patch / 2> on device buffers
// (dense.hip); A and b are host arrays, volume may be null.
int dense_sweep_check(int64_t h, int64_t w, int32_t S, const double *A, const double *b,
                      const double *depths, int64_t D, int32_t patch, double min_var,
                      bool with_volume);
void dense_sweep_launch(hipStream_t s, const uint8_t *ref, const uint8_t *src, int64_t h,
                        int64_t w, int32_t S, const double *A, const double *b,
                        const double *depths, int64_t D, int32_t patch, double min_var,
                        int32_t *index, float *delta, float *score, uint8_t *nvalid,
                        float *volume);
// The argument rules the mesh calls share (RS_EINVAL with a message, else RS_OK) and the exclusive
// scan of the int32 v[0 .. n) in place on stream s, n >= 1, the total in v[n]; sums is scratch of
// blocks(n, RS_MESH_SCAN_CHUNK) + 1 items (mesh.hip).
int mesh_check(const rs_ctx *c, const int32_t *faces, int64_t nf, int64_t nv);
void mesh_scan(hipStream_t s, int32_t *v, int64_t n, int32_t *sums);
int fmatrix_stls_lsq(rs_ctx *c, const double *pl, const double *pr, int64_t n, double *F_out);
// The two descriptor kernels of rs_cloud_fpfh (global_reg.hip) on the lists knn_run left on the
// device (`rows` wide, k + 1), enqueued on the context's stream: spfh (n, 33) and pairs (n) are
// scratch, out (n, 33) the descriptors; and, after the stream has been waited for, their timing.
void fpfh_launch(rs_ctx *c, const double *pts, const double *normals, int64_t n, int rows,
                 const int32_t *idx, const double *d2, const int32_t *count, int32_t *spfh,
                 int32_t *pairs, double *out);
int fpfh_read_timing(rs_ctx *c);
}  // namespace rs
