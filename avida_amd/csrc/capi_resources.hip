// capi_resources.hip -- resources: loading, seeding, setting and reading them.
#include "host.h"

using namespace avh;

// (the kernels: resources.hip; DESIGN.md "Resources")
// initial amounts of this world's cells (cResourceCount::Setup: RateAll(
// initial / size) + StateAll, main/cResourceCount.cc:323-328; SetCellList:
// Rate + State, main/cSpatialResCount.cc:216-231; a strip tile seeds its rows)
int avh::res_seed(avgpu_world* w) {
  DevWorld& W = w->W;
  HIPCHK(hipStreamSynchronize(w->stream));   // res_param may still be in flight
  const int64_t n = W.n, nglobal = (int64_t)W.world_x * W.world_y;
  const int nres = (int)w->res_spec.size();
  ResParam P[AVGPU_MAX_RESOURCES];
  COPY_SYNC(w, P, W.res_param, sizeof(P), hipMemcpyDeviceToHost);
  double glob[AVGPU_MAX_RESOURCES];
  memset(glob, 0, sizeof(glob));
  if (W.n_spatial) {
    std::vector<double> amt((size_t)W.n_spatial * n);
    for (int r = 0; r < nres; r++) {
      if (P[r].slot < 0) continue;
      const double per = w->res_spec[r].initial / (double)nglobal;
      for (int64_t c = 0; c < n; c++) amt[(size_t)P[r].slot * n + c] = 0.0 + per;
    }
    for (const avgpu_cell_resource& e : w->cell_spec) {
      const int64_t l = e.cell - W.cell0;
      if (e.cell >= 0 && e.cell < nglobal && l >= 0 && l < n) {
        double& a = amt[(size_t)P[e.resource].slot * n + l];
        a = a + (0.0 + e.initial);
      }
    }
    HIPCHK(hipMemcpyAsync(W.res_amount, amt.data(), amt.size() * sizeof(double), hipMemcpyHostToDevice, w->stream));
  }
  for (int r = 0; r < nres; r++) glob[r] = P[r].slot < 0 ? w->res_spec[r].initial : 0.0;
  HIPCHK(hipMemcpyAsync(W.res_global, glob, sizeof(glob), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipMemsetAsync(W.res_cons, 0, AVGPU_MAX_RESOURCES * sizeof(unsigned long long), w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  W.res_first = 1;
  return 0;
}

extern "C" {

int avgpu_load_resources(avgpu_world* w, int nres, const avgpu_resource* res, int ncell,
                         const avgpu_cell_resource* cells) {
  if (!w || nres < 0 || nres > AVGPU_MAX_RESOURCES || ncell < 0 || (ncell && !cells) || (nres && !res))
    return fail(AVGPU_EINVAL, "resource arguments");
  DevWorld& W = w->W;
  int nsp = 0;
  ResParam P[AVGPU_MAX_RESOURCES];
  memset(P, 0, sizeof(P));
  for (int r = 0; r < nres; r++) {
    const avgpu_resource& q = res[r];
    if (q.geometry < 0 || q.geometry > 2) return fail(AVGPU_EINVAL, "resource geometry");
    if (q.initial < 0 || q.inflow < 0 || q.outflow < 0 || q.outflow > 1)
      return fail(AVGPU_EINVAL, "resource initial / inflow / outflow out of range");
    ResParam& p = P[r];
    p.geometry = q.geometry;
    p.slot = q.geometry == AVGPU_RES_GLOBAL ? -1 : nsp++;
    p.in_x1 = q.inflow_x1; p.in_x2 = q.inflow_x2; p.in_y1 = q.inflow_y1; p.in_y2 = q.inflow_y2;
    p.out_x1 = q.outflow_x1; p.out_x2 = q.outflow_x2; p.out_y1 = q.outflow_y1; p.out_y2 = q.outflow_y2;
    const double decay = 1.0 - q.outflow;                        // cPopulation.cc:440
    // Source: amount / cells of the inflow rectangle (cSpatialResCount.cc:341-353)
    const double boxcells = (double)(p.in_y2 - p.in_y1 + 1) * (double)(p.in_x2 - p.in_x1 + 1) * 1.0;
    p.in_share = q.inflow / boxcells;
    p.sink_frac = 1.0 - decay;
    p.has_sink = (p.out_x1 != AVGPU_RES_NONE && p.out_y1 != AVGPU_RES_NONE &&
                  p.out_x2 != AVGPU_RES_NONE && p.out_y2 != AVGPU_RES_NONE) ? 1 : 0;
    p.xdiffuse = q.xdiffuse; p.ydiffuse = q.ydiffuse; p.xgravity = q.xgravity; p.ygravity = q.ygravity;
    p.flows = (q.xdiffuse != 0.0 || q.ydiffuse != 0.0 || q.xgravity != 0.0 || q.ygravity != 0.0) ? 1 : 0;
    p.in_all = (p.in_x2 - p.in_x1 + 1 == W.world_x && p.in_y2 - p.in_y1 + 1 == W.world_y) ? 1 : 0;
    p.out_all = (p.out_x2 - p.out_x1 + 1 == W.world_x && p.out_y2 - p.out_y1 + 1 == W.world_y) ? 1 : 0;
    // precalc tables (cResourceCount.cc:336-345), the reference's own loop
    const double step_decay = std::pow(decay, 1.0 / 10000.0), step_inflow = q.inflow * (1.0 / 10000.0);
    double dp = 1.0, ip = 0.0;
    for (int i = 1; i <= 100; i++) {
      dp = dp * step_decay;
      ip = ip * step_decay + step_inflow;
      if (i == 99) { p.decay99 = dp; p.inflow99 = ip; }
    }
    p.decay100 = dp; p.inflow100 = ip;
    w->res_geom[r] = q.geometry;
    W.res_spatial_host[r] = q.geometry != AVGPU_RES_GLOBAL;
    W.res_flows_host[r] = (int8_t)p.flows;
    W.res_grav_host[r] = (int8_t)(q.xgravity != 0.0 || q.ygravity != 0.0);
    W.res_cells_host[r] = 0;
  }
  for (int i = 0; i < ncell; i++) {
    if (cells[i].resource < 0 || cells[i].resource >= nres || res[cells[i].resource].geometry == AVGPU_RES_GLOBAL)
      return fail(AVGPU_EINVAL, "CELL entry names a resource that is not spatial");
    W.res_cells_host[cells[i].resource] = 1;
  }
  const int64_t n = W.n;
  if ((int64_t)W.world_x * W.world_y >= (int64_t)1 << 31)
    return fail(AVGPU_EUNSUPPORTED, "resources need fewer than 2^31 cells in the world");
  int rc = 0;
  // (alloc's zero fill is not relied on: res_seed writes every amount the first
  // update reads, the spatial step writes res_amount_alt and res_delta before
  // it reads them)
  if (nsp && !W.res_amount &&
      ((rc = w->alloc(&W.res_amount, (size_t)AVGPU_MAX_RESOURCES * n)) < 0 ||
       (rc = w->alloc(&W.res_amount_alt, (size_t)AVGPU_MAX_RESOURCES * n)) < 0 ||
       (rc = w->alloc(&W.res_delta, (size_t)res_delta_words(n))) < 0))
    return rc;
  // each cell's consumption in a step (newborn credit), zero at first
  if (nres && !W.cons && (rc = w->alloc(&W.cons, (size_t)AVGPU_MAX_RESOURCES * n)) < 0) return rc;
  if (ncell) {
    HIPCHK(hipStreamSynchronize(w->stream));   // no queued update still reads the last load's entries
    if ((rc = w->res_cells.alloc(ncell)) < 0) return rc;
    W.res_cells = w->res_cells.get();
    HIPCHK(hipMemcpyAsync(W.res_cells, cells, ncell * sizeof(avgpu_cell_resource), hipMemcpyHostToDevice, w->stream));
  }
  W.n_res = nres;
  W.n_cellres = ncell;
  W.n_spatial = nsp;
  w->res_spec.assign(res, res + nres);
  w->cell_spec.assign(cells, cells + ncell);
  HIPCHK(hipMemcpyAsync(W.res_param, P, sizeof(P), hipMemcpyHostToDevice, w->stream));
  return res_seed(w);
}

int avgpu_set_resources(avgpu_world* w, const double* levels, const double* spatial) {
  if (!w || !levels) return fail(AVGPU_EINVAL, "args");
  DevWorld& W = w->W;
  double glob[AVGPU_MAX_RESOURCES];
  ResParam P[AVGPU_MAX_RESOURCES];
  COPY_SYNC(w, glob, W.res_global, sizeof(glob), hipMemcpyDeviceToHost);
  COPY_SYNC(w, P, W.res_param, sizeof(P), hipMemcpyDeviceToHost);
  for (int r = 0; r < W.n_res; r++) {
    if (P[r].slot < 0) { glob[r] = levels[r]; continue; }
    if (!spatial) return fail(AVGPU_EINVAL, "spatial resources need their grids");
    COPY_SYNC(w, W.res_amount + (size_t)P[r].slot * W.n, spatial + (size_t)r * W.n, W.n * sizeof(double),
              hipMemcpyHostToDevice);
  }
  COPY_SYNC(w, W.res_global, glob, sizeof(glob), hipMemcpyHostToDevice);
  SET_SYNC(w, W.res_cons, 0, AVGPU_MAX_RESOURCES * sizeof(unsigned long long));
  W.res_first = 0;
  return 0;
}

int avgpu_get_resources(avgpu_world* w, double* levels, double* spatial) {
  if (!w || !levels) return fail(AVGPU_EINVAL, "args");
  DevWorld& W = w->W;
  double glob[AVGPU_MAX_RESOURCES];
  ResParam P[AVGPU_MAX_RESOURCES];
  COPY_SYNC(w, glob, W.res_global, sizeof(glob), hipMemcpyDeviceToHost);
  COPY_SYNC(w, P, W.res_param, sizeof(P), hipMemcpyDeviceToHost);
  std::vector<double> row(W.n);
  for (int r = 0; r < W.n_res; r++) {
    if (P[r].slot < 0) {
      levels[r] = glob[r];
      if (spatial) memset(spatial + (size_t)r * W.n, 0, W.n * sizeof(double));
      continue;
    }
    COPY_SYNC(w, row.data(), W.res_amount + (size_t)P[r].slot * W.n, W.n * sizeof(double),
              hipMemcpyDeviceToHost);
    double sum = 0.0;                                   // cStats::PrintResourceData order
    for (int64_t c = 0; c < W.n; c++) sum += row[c];
    levels[r] = sum;
    if (spatial) memcpy(spatial + (size_t)r * W.n, row.data(), W.n * sizeof(double));
  }
  return 0;
}

}  // extern "C"
