// capi_tiles.hip -- strip tiles (DESIGN.md "Multi-GPU").
#include "host.h"

using namespace avh;

extern "C" {

int avgpu_set_tile(avgpu_world* w, int64_t row0, int64_t arena_bytes) {
  if (w && (w->cfg.birth_method == 1 || w->cfg.birth_method == 2))
    return fail(AVGPU_EUNSUPPORTED, "BIRTH_METHOD 1 / 2 on strip tiles (the ghost rows carry no age or merit)");
  if (w && (w->cfg.birth_method == 4 || w->cfg.birth_method == 5))
    return fail(AVGPU_EUNSUPPORTED, "BIRTH_METHOD 4 / 5 on strip tiles (a soup birth may land in any strip)");
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  DevWorld& W = w->W;
  const int64_t X = W.world_x;
  if (X <= 0 || W.n % X) return fail(AVGPU_EINVAL, "tile cells must be whole rows of WORLD_X");
  const int64_t rows = W.n / X;
  if (rows < 2) return fail(AVGPU_EINVAL, "a tile needs at least 2 rows");
  if (W.n % 256) return fail(AVGPU_EINVAL, "tile cells must be a multiple of 256 (merit blocks)");
  if (row0 < 0 || row0 + rows > W.global_rows)
    return fail(AVGPU_EINVAL, "tile rows outside WORLD_Y (the global row count)");
  if (arena_bytes <= 0) arena_bytes = std::max<int64_t>(256 * 1024, X * 256);
  arena_bytes = (arena_bytes + 15) / 16 * 16;
  W.row0 = (int32_t)row0;
  W.rows = (int32_t)rows;
  W.tiled = rows < W.global_rows ? 1 : 0;
  W.cell0 = row0 * X;
  W.r_arena = arena_bytes;
  w->tile_buffers = false;
  W.rs_send[0] = W.rs_send[1] = W.rs_recv[0] = W.rs_recv[1] = nullptr;
  if (W.n_res) return res_seed(w);   // this strip's share of the initial amounts
  return 0;
}

int avgpu_tile_res_bytes(avgpu_world* w, int64_t* bytes) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if (bytes) *bytes = (int64_t)w->W.n_spatial * w->W.world_x * (int64_t)sizeof(double);
  return 0;
}

int avgpu_set_tile_res_buffers(avgpu_world* w, void* send_up, void* send_down, void* recv_up,
                               void* recv_down) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if (!w->W.tiled) return fail(AVGPU_ESTATE, "avgpu_set_tile did not make this world a strip tile");
  if (w->W.n_spatial && (!send_up || !send_down || !recv_up || !recv_down))
    return fail(AVGPU_EINVAL, "NULL tile resource buffer");
  DevWorld& W = w->W;
  W.rs_send[0] = (double*)send_up; W.rs_send[1] = (double*)send_down;
  W.rs_recv[0] = (double*)recv_up; W.rs_recv[1] = (double*)recv_down;
  return 0;
}

int avgpu_tile_res_cons(avgpu_world* w, uint64_t* dev_out) {
  int rc = ready(w);
  if (rc < 0) return rc;
  if (!dev_out) return fail(AVGPU_EINVAL, "dev_out is NULL");
  HIPCHK(hipMemcpyAsync(dev_out, w->W.res_cons, AVGPU_MAX_RESOURCES * sizeof(unsigned long long),
                        hipMemcpyDeviceToDevice, w->stream));
  int g = 0;
  for (int r = 0; r < w->W.n_res; r++) g += w->res_geom[r] == AVGPU_RES_GLOBAL;
  return g;
}

int avgpu_tile_res_settle(avgpu_world* w, const uint64_t* dev_sum) {
  int rc = ready(w);
  if (rc < 0) return rc;
  if (!dev_sum) return fail(AVGPU_EINVAL, "dev_sum is NULL");
  launch_resources_settle(w->W, w->stream, (const unsigned long long*)dev_sum);
  HIPCHK(hipGetLastError());
  return 0;
}

int avgpu_tile_buffer_bytes(avgpu_world* w, int64_t* partial_bytes, int64_t* halo_b, int64_t* record_b) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if (partial_bytes) *partial_bytes = tile_part_stride((w->W.n + 255) / 256) * (int64_t)sizeof(double);
  if (halo_b) *halo_b = halo_bytes(w->W.world_x);
  if (record_b) *record_b = record_bytes(w->W.world_x, w->W.r_arena);
  return 0;
}

int avgpu_set_tile_buffers(avgpu_world* w, void* halo_send_up, void* halo_send_down, void* halo_recv_up,
                           void* halo_recv_down, void* rec_send_up, void* rec_send_down,
                           void* rec_recv_up, void* rec_recv_down) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if (!w->W.tiled) return fail(AVGPU_ESTATE, "avgpu_set_tile did not make this world a strip tile");
  void* p[8] = {halo_send_up, halo_send_down, halo_recv_up, halo_recv_down,
                rec_send_up, rec_send_down, rec_recv_up, rec_recv_down};
  for (int i = 0; i < 8; i++)
    if (!p[i]) return fail(AVGPU_EINVAL, "NULL tile buffer");
  DevWorld& W = w->W;
  W.h_send[0] = (uint8_t*)p[0]; W.h_send[1] = (uint8_t*)p[1];
  W.h_recv[0] = (uint8_t*)p[2]; W.h_recv[1] = (uint8_t*)p[3];
  W.r_send[0] = (uint8_t*)p[4]; W.r_send[1] = (uint8_t*)p[5];
  W.r_recv[0] = (uint8_t*)p[6]; W.r_recv[1] = (uint8_t*)p[7];
  w->tile_buffers = true;
  return 0;
}

static int tile_ready(avgpu_world* w) {
  int rc = ready(w);
  if (rc < 0) return rc;
  if (!w->W.tiled || !w->tile_buffers) return fail(AVGPU_ESTATE, "not a strip tile with registered buffers");
  return 0;
}

int avgpu_tile_partials(avgpu_world* w, double* dev_out) {
  int rc = ready(w);
  if (rc < 0) return rc;
  if (!dev_out) return fail(AVGPU_EINVAL, "dev_out is NULL");
  // a strip's first step of an update clears the update's counters, a later
  // step its queues only (the counts add up over the update)
  launch_tile_partials(w->W, w->stream, dev_out,
                       w->W.tiled ? (w->tile_sub_next == 0 ? RESET_COUNTS : RESET_QUEUES) : RESET_NONE);
  if (w->W.tiled) launch_resources_pack(w->W, w->stream);
  HIPCHK(hipGetLastError());
  return 0;
}

// the update's batch steps from every strip's predictor (the gathered
// partials' tails) and the organisms of the last step (the same on every strip)
int avgpu_tile_steps(avgpu_world* w, const double* dev_gathered, int ntiles, int* k_out) {
  int rc = tile_ready(w);
  if (rc < 0) return rc;
  if (!dev_gathered || ntiles < 1 || !k_out) return fail(AVGPU_EINVAL, "gathered partials / k_out");
  const int64_t nb = (w->W.n + 255) / 256, stride = tile_part_stride(nb);
  std::vector<double> tail((size_t)(TAIL_WORDS * ntiles));
  for (int k = 0; k < ntiles; k++)
    HIPCHK(hipMemcpyAsync(tail.data() + TAIL_WORDS * k, dev_gathered + k * stride + tile_tail_off(nb),
                          TAIL_WORDS * sizeof(double), hipMemcpyDeviceToHost, w->stream));
  double n = 0.0;
  HIPCHK(hipMemcpyAsync(&n, w->d_totals + TOT_ORGS, sizeof(double), hipMemcpyDeviceToHost, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  long long sum = 0, bins[4] = {0, 0, 0, 0};
  for (int k = 0; k < ntiles; k++) {
    long long v;
    memcpy(&v, tail.data() + TAIL_WORDS * k + TAIL_PRED, 8);
    sum += v;
    for (int q = 0; q < 4; q++) {
      long long c;
      memcpy(&c, tail.data() + TAIL_WORDS * k + TAIL_QUARTER0 + q, 8);
      bins[q] += c;
    }
  }
  const long long dens = std::max(std::max(bins[0], bins[1]), std::max(bins[2], bins[3]));
  *k_out = choose_k(w->cfg, sum, (long long)n, false, dens);
  return 0;
}

int avgpu_tile_begin_step(avgpu_world* w, const double* dev_gathered, int ntiles, int sub, int K) {
  int rc = tile_ready(w);
  if (rc < 0) return rc;
  if (w->W.n_spatial && !w->W.rs_recv[0])
    return fail(AVGPU_ESTATE, "spatial resources need avgpu_set_tile_res_buffers");
  if (!dev_gathered || ntiles < 1) return fail(AVGPU_EINVAL, "gathered partials");
  if (K < 1 || K > 64 || sub < 0 || sub >= K) return fail(AVGPU_EINVAL, "batch step sub of K");
  if (K > 1 && w->cfg.slicing_method != AVGPU_SLICE_PROBABILISTIC)
    return fail(AVGPU_EUNSUPPORTED, "batch steps > 1 need SLICING_METHOD 1");
  // the scheduler's top tree spans every strip's blocks
  {
    int64_t P = 1;
    const int64_t nbt = ((w->W.n + 255) / 256) * (int64_t)ntiles;
    while (P < nbt) P <<= 1;
    if (P > w->W.tree_cap) {   // (the smaller buffers stay in the world's allocations)
      if ((rc = w->alloc(&w->W.tree_scr, (size_t)(2 * P))) < 0) return rc;
      if ((rc = w->alloc(&w->W.tree_cnt, (size_t)(2 * P))) < 0) return rc;
      w->W.tree_cap = P;
      const int prc = push_world(w);
      if (prc < 0) return prc;
    }
  }
  // (the counters were cleared by avgpu_tile_partials' launch at step 0)
  const uint32_t key = step_key(w, sub, K);
  launch_tile_pre(w->W, w->stream, dev_gathered, ntiles, w->d_totals, key, sub, K);
  if (sub == 0) after_resources_begin(w);
  HIPCHK(hipGetLastError());
  rc = interpret(w, AVGPU_MODE_WORLD, 0, w->W.n, true);
  if (rc < 0) return rc;
  launch_tile_after_interpret(w->W, w->stream);
  HIPCHK(hipGetLastError());
  w->ntiles_last = ntiles;
  w->tile_sub = sub; w->tile_k = K; w->tile_key = key;
  w->tile_sub_next = sub + 1 < K ? sub + 1 : 0;
  return 0;
}

int avgpu_tile_begin(avgpu_world* w, const double* dev_gathered, int ntiles) {
  return avgpu_tile_begin_step(w, dev_gathered, ntiles, 0, 1);
}

int avgpu_tile_place(avgpu_world* w, int round, int phase) {
  int rc = tile_ready(w);
  if (rc < 0) return rc;
  if (round < 0 || round > 3 || phase < 0 || phase > 3 || (phase >= 1 && phase <= 2 && round != 3) ||
      (phase == 3 && round != 0))
    return fail(AVGPU_EINVAL, "round 0..3 with phase 0, round 0 with phase 3; phases 1, 2 after round 3");
  launch_tile_place(w->W, w->stream, round, phase, w->tile_key, w->tile_sub, w->tile_k);
  HIPCHK(hipGetLastError());
  return 0;
}

int avgpu_tile_finish(avgpu_world* w, avgpu_update_stats* out) {
  int rc = tile_ready(w);
  if (rc < 0) return rc;
  // the received offspring, the step's newborn pass; after the update's last
  // step its statistics
  launch_tile_finish(w->W, w->stream, w->tile_key, w->tile_sub, w->tile_k);
  launch_newborns(w->W, w->d_W, w->stream);
  HIPCHK(hipGetLastError());
  if (w->tile_sub + 1 < w->tile_k) return 0;
  if (out) launch_stats(w->W, w->stream, w->d_stats);
  HIPCHK(hipGetLastError());
  w->stats_stale = out == nullptr;
  w->last_k = w->tile_k;
  w->update++;
  if (out) return avgpu_get_stats(w, out);
  return 0;
}

}  // extern "C"
