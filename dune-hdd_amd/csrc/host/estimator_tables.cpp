// dune-hdd_amd/csrc/host/estimator_tables.cpp -- host tables of the ESV2007 estimator (hdd_estimator_create): the
// vertex patches the Oswald interpolation gathers through and the boundary-vertex flags, built once per mesh from the
// host view; and the per-segment tables of the OS2014 block estimator (hdd_estimator_set_segments): bounds, chunk
// prefix, diameters.  Pure host code: the scope checks of the estimator answer here, without a device.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
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
  out->vertex_coords.resize(size_t(2 * nv));   // (kept with ev for the segment diameters: the same one pass)
  if (int rc = hdd_local_vertices(l, &nv, ev.data(), out->vertex_coords.data())) return rc;
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
  out->elem_vertices.swap(ev);
  return HDD_OK;
}

namespace {
struct Pt {
  double x, y;
};

// z of (a - o) x (b - o)
inline double cross(const Pt& o, const Pt& a, const Pt& b) { return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x); }

// the largest distance between two of the points (sorted in place): the pairwise maximum over their convex hull by
// the monotone chain.  Collinear points leave the hull (a rectangle keeps its four corners), which keeps its extreme
// points: the maximum is attained there.
double diameter(std::vector<Pt>& pts, std::vector<Pt>& hull)
{
  std::sort(pts.begin(), pts.end(), [](const Pt& a, const Pt& b) { return a.x < b.x || (a.x == b.x && a.y < b.y); });
  const size_t n = pts.size();
  hull.clear();
  if (n < 3) hull = pts;
  else {
    hull.resize(2 * n);
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) {   // lower chain
      while (k >= 2 && cross(hull[k - 2], hull[k - 1], pts[i]) <= 0.0) --k;
      hull[k++] = pts[i];
    }
    for (size_t i = n - 1, lower = k + 1; i-- > 0;) {   // upper chain
      while (k >= lower && cross(hull[k - 2], hull[k - 1], pts[i]) <= 0.0) --k;
      hull[k++] = pts[i];
    }
    hull.resize(k - 1);   // the last point is the first again
  }
  double d = 0.0;
  for (size_t i = 0; i < hull.size(); ++i)
    for (size_t j = i + 1; j < hull.size(); ++j) {
      const double dx = hull[i].x - hull[j].x, dy = hull[i].y - hull[j].y;
      d = std::max(d, std::sqrt(dx * dx + dy * dy));
    }
  return d;
}
}  // namespace

bool theta_positive(int32_t n_comp, const double* theta)
{
  for (int q = 0; q < n_comp; ++q)
    if (!(theta[q] > 0.0)) return false;
  return true;
}

int estimator_segment_tables(int64_t n_local, int64_t n_vertices, const int32_t* elem_vertices, const double* vertex_coords,
                             int64_t n_segments, const int64_t* bounds, SegmentTables* out)
{
  static const char* who = "hdd_estimator_set_segments: ";
  if (n_segments < 0) return set_error(HDD_ERR_INVALID, std::string(who) + "n_segments is negative");
  if (!bounds) return set_error(HDD_ERR_INVALID, std::string(who) + "null bounds");
  if (n_segments > n_local)
    return set_error(HDD_ERR_INVALID, std::string(who) + "more segments than elements (every segment holds an element)");
  if (bounds[0] != 0) return set_error(HDD_ERR_INVALID, std::string(who) + "bounds[0] is not 0");
  for (int64_t s = 0; s < n_segments; ++s)
    if (bounds[s + 1] <= bounds[s])
      return set_error(HDD_ERR_INVALID, std::string(who) + "bounds are not strictly ascending (segment " +
                                            std::to_string(s) + ")");
  if (bounds[n_segments] != n_local)
    return set_error(HDD_ERR_INVALID, std::string(who) + "bounds[n_segments] is not the number of elements: the segments "
                                                          "partition [0, n)");
  out->bounds.assign(bounds, bounds + n_segments + 1);
  out->chunk_prefix.assign(size_t(n_segments + 1), 0);
  out->diam.assign(size_t(n_segments), 0.0);
  std::vector<int64_t> seen(size_t(n_vertices), -1);   // the last segment that met the vertex
  std::vector<Pt> pts, hull;
  for (int64_t s = 0; s < n_segments; ++s) {
    out->chunk_prefix[s + 1] = out->chunk_prefix[s] + (bounds[s + 1] - bounds[s] + 255) / 256;
    pts.clear();
    for (int64_t e = bounds[s]; e < bounds[s + 1]; ++e)
      for (int i = 0; i < 3; ++i) {
        const int32_t v = elem_vertices[i * n_local + e];
        if (seen[v] == s) continue;
        seen[v] = s;
        pts.push_back(Pt{vertex_coords[2 * int64_t(v)], vertex_coords[2 * int64_t(v) + 1]});
      }
    out->diam[s] = diameter(pts, hull);
  }
  return HDD_OK;
}

}  // namespace hdd
