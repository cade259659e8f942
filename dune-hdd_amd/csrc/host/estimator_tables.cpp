// dune-hdd_amd/csrc/host/estimator_tables.cpp -- host tables of the ESV2007 estimator (hdd_estimator_create): the
// vertex patches the Oswald interpolation gathers through and the boundary-vertex flags, built once per mesh from the
// host view.  Pure host code: the scope checks of the estimator answer here, without a device.
#include <cstdint>
#include <vector>

#include "hdd.h"
#include "hdd_internal.hh"

namespace hdd {

int estimator_tables(const hdd_local* l, EstimatorTables* out)
{
  static const char* who = "hdd_estimator_create: ";
  if (local_elem_type(l) != HDD_SIMPLEX)
    return set_error(HDD_ERR_UNSUPPORTED, std::string(who) + "the ESV2007 estimator needs a 2d conforming simplex grid");
  hdd_local_info info;
  if (int rc = hdd_local_get_info(l, &info)) return rc;
  if (info.n_ghost != 0 || info.own_begin != 0 || info.own_end != info.n_local)
    return set_error(HDD_ERR_UNSUPPORTED, std::string(who) + "whole-grid view only (a vertex patch needs every element "
                                                                "around the vertex; this view has ghosts)");
  const int64_t n = info.n_local;
  if (3 * n >= (int64_t(1) << 31))
    return set_error(HDD_ERR_UNSUPPORTED, std::string(who) + "more than 2^31 / 3 elements");
  std::vector<int32_t> nbrs(size_t(3 * n));
  if (int rc = hdd_local_fill(l, nullptr, nbrs.data(), nullptr, nullptr, nullptr)) return rc;
  for (int64_t k = 0; k < 3 * n; ++k)
    if (nbrs[k] == HDD_NBR_NEUMANN)
      return set_error(HDD_ERR_UNSUPPORTED, std::string(who) + "Neumann faces are not covered (the Oswald interpolation "
                                                                  "assumes Dirichlet data on the whole boundary)");
  int64_t nv = 0;
  if (int rc = hdd_local_vertices(l, &nv, nullptr, nullptr)) return rc;
  std::vector<int32_t> ev(size_t(3 * n));
  if (int rc = hdd_local_vertices(l, &nv, ev.data(), nullptr)) return rc;
  out->n_local = n;
  out->n_vertices = nv;
  out->patch_ptr.assign(size_t(nv + 1), 0);
  for (int64_t k = 0; k < 3 * n; ++k) out->patch_ptr[size_t(ev[k]) + 1]++;
  for (int64_t v = 0; v < nv; ++v) out->patch_ptr[v + 1] += out->patch_ptr[v];
  out->patch_dof.resize(size_t(3 * n));
  std::vector<int64_t> pos(out->patch_ptr.begin(), out->patch_ptr.end() - 1);
  for (int64_t e = 0; e < n; ++e)        // element-major: the DoFs of a vertex come out ascending
    for (int i = 0; i < 3; ++i) out->patch_dof[size_t(pos[ev[i * n + e]]++)] = int32_t(3 * e + i);
  out->vertex_bnd.assign(size_t(nv), 0);
  static const int FV[3][2] = {{0, 1}, {0, 2}, {1, 2}};
  for (int f = 0; f < 3; ++f)
    for (int64_t e = 0; e < n; ++e)
      if (nbrs[f * n + e] < 0) {
        out->vertex_bnd[ev[FV[f][0] * n + e]] = 1;
        out->vertex_bnd[ev[FV[f][1] * n + e]] = 1;
      }
  return HDD_OK;
}

}  // namespace hdd
