// dune-hdd_amd/csrc/kernels/shard.hip
//
// Sharded BlockSWIPDG behind the C ABI (SURVEY.md 8(b) hdd_block_assemble_sharded, 8(e)).
//
// The reference assembles BlockSWIPDG sequentially over subdomains (block-swipdg.hh:271, 334): the local
// operator of ss, the boundary terms of a domain-boundary subdomain (assemble_boundary_contributions,
// 1136-1179) and, for each neighbour nn > ss, the SWIPDG::Inner coupling into A_ss, A_ss,nn, A_nn,ss, A_nn
// (assemble_coupling_contributions, 1270-1326).  Here one rank (process or thread, one GPU each) owns a
// contiguous subdomain range and writes exactly the rows of its elements -- the rows of A_ss and A_ss,nn
// (block-swipdg.hh:355-382) -- computing both sides of every face it touches (owner-computes), so no
// matrix entry is ever summed across ranks.  The only exchange is the face halo: the per-element records
// (diffusion tensor, per-element diffusion factors [, vertex coordinates]) of the ghost elements.
//
// This file: the shard itself -- its rank-local mesh, halo plan and tile lists, built once (hdd_shard_create),
// and the getters.  The step is shard_step.hip, the communicators comm.hip.
#include <algorithm>

#include "shard_internal.hh"

using hdd::set_error;
using namespace hdd::shard;

namespace {

template <class T>
hipError_t upload(T** d, const std::vector<T>& h)
{
  *d = nullptr;
  if (h.empty()) return hipSuccess;
  hipError_t e = hipMalloc(d, h.size() * sizeof(T));
  if (e != hipSuccess) return e;
  return hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

}  // namespace

extern "C" void hdd_shard_destroy(hdd_shard* sh)
{
  if (!sh) return;
  if (!sh->host_only) (void)hipSetDevice(sh->device);
  if (sh->aux) (void)hipStreamDestroy(sh->aux);
  if (sh->ev_in) (void)hipEventDestroy(sh->ev_in);
  if (sh->ev_out) (void)hipEventDestroy(sh->ev_out);
  if (sh->ev_mark) (void)hipEventDestroy(sh->ev_mark);
  if (sh->ev_pack) (void)hipEventDestroy(sh->ev_pack);
  if (sh->ev_xdone) (void)hipEventDestroy(sh->ev_xdone);
  for (void* p : {static_cast<void*>(sh->d_coords), static_cast<void*>(sh->d_nbrs), static_cast<void*>(sh->d_finfo),
                  static_cast<void*>(sh->d_gid), static_cast<void*>(sh->d_send_idx), static_cast<void*>(sh->d_sbuf),
                  static_cast<void*>(sh->d_rbuf), static_cast<void*>(sh->d_tiles_in),
                  static_cast<void*>(sh->d_tiles_bd), static_cast<void*>(sh->d_ev), static_cast<void*>(sh->d_vxy),
                  static_cast<void*>(sh->d_fix), static_cast<void*>(sh->d_fixbuf)})
    if (p) (void)hipFree(p);
  if (sh->local) hdd_local_destroy(sh->local);
  delete sh;
}

extern "C" int hdd_shard_create(hdd_ctx* ctx, const hdd_grid* g, int32_t nranks, int32_t rank, const int32_t* owner,
                                hdd_shard** out)
{
  if (!g || !out || nranks < 1 || rank < 0 || rank >= nranks)
    return set_error(HDD_ERR_INVALID, "hdd_shard_create: invalid argument");
  hdd_grid_info gi{};
  int rc = hdd_grid_get_info(g, &gi);
  if (rc) return rc;
  std::vector<int32_t> own(size_t(gi.n_subdomains));
  if (owner) {
    std::copy(owner, owner + gi.n_subdomains, own.begin());
  } else {
    if (nranks > gi.n_subdomains)
      return set_error(HDD_ERR_INVALID, "hdd_shard_create: more ranks than subdomains");
    for (int32_t r = 0; r < nranks; ++r)
      for (int64_t s = int64_t(r) * gi.n_subdomains / nranks; s < int64_t(r + 1) * gi.n_subdomains / nranks; ++s)
        own[size_t(s)] = r;
  }
  int32_t s0 = -1, s1 = -1;
  for (int32_t s = 0; s < gi.n_subdomains; ++s) {
    if (own[s] < 0 || own[s] >= nranks) return set_error(HDD_ERR_RANGE, "hdd_shard_create: owner out of range");
    if (own[s] != rank) continue;
    if (s0 < 0) s0 = s;
    else if (s1 != s) return set_error(HDD_ERR_UNSUPPORTED, "hdd_shard_create: owned subdomains must be contiguous");
    s1 = s + 1;
  }
  if (s0 < 0) return set_error(HDD_ERR_INVALID, "hdd_shard_create: rank owns no subdomain");

  auto* sh = new hdd_shard;
  auto fail = [&](int code) {
    hdd_shard_destroy(sh);
    return code;
  };
  sh->device = hdd::ctx_device(ctx);
  sh->host_only = !ctx;
  sh->gi = gi;
  sh->rank = rank;
  sh->nranks = nranks;
  sh->s_begin = s0;
  sh->s_end = s1;
  if (gi.elem_type == HDD_HEX)
    while ((sh->degree + 1) * (sh->degree + 1) * (sh->degree + 1) < gi.nb) ++sh->degree;
  rc = hdd_local_create(g, s0, s1, &sh->local);
  if (rc) return fail(rc);
  rc = hdd_local_get_info(sh->local, &sh->li);
  if (rc) return fail(rc);
  const int64_t nl = sh->li.n_local, ob = sh->li.own_begin, oe = sh->li.own_end;
  std::vector<double> coords(size_t(gi.dim) * gi.nvpe * nl);
  std::vector<int32_t> nbrs(size_t(gi.nfaces) * nl);
  std::vector<uint32_t> finfo(static_cast<size_t>(nl));
  sh->gid.resize(size_t(nl));
  rc = hdd_local_fill(sh->local, coords.data(), nbrs.data(), finfo.data(), sh->gid.data(), nullptr);
  if (rc) return fail(rc);
  rc = hdd_dg_pattern_count(gi.nfaces, gi.nb, nl, ob, oe, nbrs.data(), &sh->nnz);
  if (rc) return fail(rc);
  // vertex-indexed geometry of the local elements (2d): what the P1 / Q1 kernels read
  std::vector<int32_t> ev;
  std::vector<double> vxy;
  if (gi.dim == 2) {
    int64_t nvl = 0;
    rc = hdd_local_vertices(sh->local, &nvl, nullptr, nullptr);
    if (rc) return fail(rc);
    ev.resize(size_t(gi.nvpe) * nl);
    vxy.resize(size_t(2) * nvl);
    rc = hdd_local_vertices(sh->local, &nvl, ev.data(), vxy.data());
    if (rc) return fail(rc);
  }

  // halo plan: peers ascending, send lists concatenated in peer order
  int32_t np = 0;
  rc = hdd_local_halo_plan(sh->local, own.data(), rank, &np, nullptr, nullptr, nullptr, nullptr);
  if (rc) return fail(rc);
  if (np > SH_MAX_PEERS) return fail(set_error(HDD_ERR_UNSUPPORTED, "hdd_shard_create: more than 64 halo peers"));
  sh->peers.resize(size_t(np));
  std::vector<int64_t> sc(static_cast<size_t>(np)), ro(static_cast<size_t>(np)), rcnt(static_cast<size_t>(np));
  rc = hdd_local_halo_plan(sh->local, own.data(), rank, &np, sh->peers.data(), sc.data(), ro.data(), rcnt.data());
  if (rc) return fail(rc);
  sh->send_prefix.assign(size_t(np) + 1, 0);
  sh->recv_prefix.assign(size_t(np) + 1, 0);
  sh->recv_col0 = ro;
  for (int32_t k = 0; k < np; ++k) {
    sh->send_prefix[k + 1] = sh->send_prefix[k] + sc[k];
    sh->recv_prefix[k + 1] = sh->recv_prefix[k] + rcnt[k];
  }
  std::vector<int32_t> send_idx(size_t(sh->send_prefix[np]));
  for (int32_t k = 0; k < np; ++k) {
    if (!sc[k]) continue;
    rc = hdd_local_send_list(sh->local, own.data(), rank, k, send_idx.data() + sh->send_prefix[k]);
    if (rc) return fail(rc);
  }

  // interior / halo-boundary tiles (64 owned elements; a boundary tile has an element with a ghost face)
  const int64_t n_own = oe - ob;
  sh->n_tiles = (n_own + 63) / 64;
  std::vector<int32_t> tin, tbd, fix;
  for (int64_t t = 0; t < sh->n_tiles; ++t) {
    bool ghost = false;
    for (int64_t e = ob + 64 * t; e < std::min(oe, ob + 64 * t + 64); ++e) {
      bool eg = false;
      for (int f = 0; f < gi.nfaces; ++f) {
        const int32_t n = nbrs[size_t(f) * nl + e];
        if (n >= 0 && (n < ob || n >= oe)) {
          eg = true;
          ++sh->halo_faces;
        }
      }
      if (eg) fix.push_back(int32_t(e - ob));
      ghost |= eg;
    }
    (ghost ? tbd : tin).push_back(int32_t(t));
  }
  sh->n_fix = int64_t(fix.size());
  sh->n_in = int64_t(tin.size());
  sh->n_bd = int64_t(tbd.size());
  sh->send_idx = send_idx;
  sh->tiles_in = tin;
  sh->tiles_bd = tbd;
  // message rows: coordinates + symmetric tensor + one row per diffusion-factor component
  sh->max_rows = gi.dim * gi.nvpe + (gi.dim == 3 ? 6 : 3) + HDD_MAX_COMP;
  if (!ctx) {   // host-only shard: plan and local mesh, nothing on a device (CPU tests of the halo protocol)
    sh->host_only = true;
    *out = sh;
    return HDD_OK;
  }

  hipError_t e = hipSetDevice(sh->device);
  if (e == hipSuccess) e = upload(&sh->d_coords, coords);
  if (e == hipSuccess) e = upload(&sh->d_nbrs, nbrs);
  if (e == hipSuccess) e = upload(&sh->d_finfo, finfo);
  if (e == hipSuccess) e = upload(&sh->d_gid, sh->gid);
  if (e == hipSuccess && !ev.empty()) e = upload(&sh->d_ev, ev);
  if (e == hipSuccess && !vxy.empty()) e = upload(&sh->d_vxy, vxy);
  if (e == hipSuccess) e = upload(&sh->d_send_idx, send_idx);
  if (e == hipSuccess) e = upload(&sh->d_tiles_in, tin);
  if (e == hipSuccess) e = upload(&sh->d_tiles_bd, tbd);
  if (e == hipSuccess) e = upload(&sh->d_fix, fix);
  if (e == hipSuccess && sh->send_prefix[np])
    e = hipMalloc(&sh->d_sbuf, size_t(sh->max_rows) * sh->send_prefix[np] * sizeof(double));
  if (e == hipSuccess && sh->recv_prefix[np])
    e = hipMalloc(&sh->d_rbuf, size_t(sh->max_rows) * sh->recv_prefix[np] * sizeof(double));
  if (e != hipSuccess) return fail(hip_fail(e, "hdd_shard_create: upload"));
  *out = sh;
  return HDD_OK;
}

extern "C" int hdd_shard_get_info(const hdd_shard* sh, hdd_shard_info* o)
{
  if (!sh || !o) return set_error(HDD_ERR_INVALID, "hdd_shard_get_info: null argument");
  o->n_local = sh->li.n_local;
  o->own_begin = sh->li.own_begin;
  o->own_end = sh->li.own_end;
  o->n_ghost = sh->li.n_ghost;
  o->global_first = sh->li.global_first;
  o->n_rows = int64_t(sh->gi.nb) * (sh->li.own_end - sh->li.own_begin);
  o->n_cols = int64_t(sh->gi.nb) * sh->gi.n_elements;
  o->nnz = sh->nnz;
  o->rank = sh->rank;
  o->nranks = sh->nranks;
  o->s_begin = sh->s_begin;
  o->s_end = sh->s_end;
  o->n_peers = int32_t(sh->peers.size());
  o->nb = sh->gi.nb;
  o->n_tiles = sh->n_tiles;
  o->n_tiles_interior = sh->n_in;
  o->n_tiles_boundary = sh->n_bd;
  o->halo_send = sh->send_prefix.back();
  o->halo_recv = sh->recv_prefix.back();
  o->halo_faces = sh->halo_faces;
  o->halo_elements = sh->n_fix;
  return HDD_OK;
}

extern "C" int hdd_shard_halo_lists(const hdd_shard* sh, int32_t* peers, int64_t* send_prefix, int32_t* send_idx,
                                    int64_t* recv_prefix, int64_t* recv_col0)
{
  if (!sh) return set_error(HDD_ERR_INVALID, "hdd_shard_halo_lists: null shard");
  const size_t np = sh->peers.size();
  if (peers) std::copy(sh->peers.begin(), sh->peers.end(), peers);
  if (send_prefix) std::copy(sh->send_prefix.begin(), sh->send_prefix.end(), send_prefix);
  if (send_idx) std::copy(sh->send_idx.begin(), sh->send_idx.end(), send_idx);
  if (recv_prefix) std::copy(sh->recv_prefix.begin(), sh->recv_prefix.end(), recv_prefix);
  if (recv_col0) std::copy(sh->recv_col0.begin(), sh->recv_col0.begin() + np, recv_col0);
  return HDD_OK;
}

extern "C" int hdd_shard_tile_lists(const hdd_shard* sh, int32_t* interior, int32_t* boundary)
{
  if (!sh) return set_error(HDD_ERR_INVALID, "hdd_shard_tile_lists: null shard");
  if (interior) std::copy(sh->tiles_in.begin(), sh->tiles_in.end(), interior);
  if (boundary) std::copy(sh->tiles_bd.begin(), sh->tiles_bd.end(), boundary);
  return HDD_OK;
}

extern "C" int hdd_shard_mesh(const hdd_shard* sh, hdd_mesh* m)
{
  if (!sh || !m) return set_error(HDD_ERR_INVALID, "hdd_shard_mesh: null argument");
  if (sh->host_only) return set_error(HDD_ERR_INVALID, "hdd_shard_mesh: host-only shard (no device mesh)");
  *m = hdd_mesh{sh->gi.elem_type, sh->gi.elem_type == HDD_HEX ? sh->degree : 1, sh->li.n_local, sh->li.own_begin,
                sh->li.own_end, sh->d_coords, sh->d_nbrs, sh->d_finfo, sh->d_ev, sh->d_vxy};
  return HDD_OK;
}

extern "C" int hdd_shard_global_ids(const hdd_shard* sh, int64_t* global_id)
{
  if (!sh || !global_id) return set_error(HDD_ERR_INVALID, "hdd_shard_global_ids: null argument");
  std::copy(sh->gid.begin(), sh->gid.end(), global_id);
  return HDD_OK;
}

extern "C" int hdd_shard_centers(const hdd_shard* sh, double* centers)
{
  if (!sh || !centers) return set_error(HDD_ERR_INVALID, "hdd_shard_centers: null argument");
  return hdd_local_centers(sh->local, centers);
}

extern "C" int hdd_shard_pattern_fill(hdd_ctx* ctx, const hdd_shard* sh, int64_t* d_row_ptr, int32_t* d_col,
                                      int64_t* d_elem_ptr, void* stream)
{
  if (!ctx || !sh || !d_row_ptr || !d_col || !d_elem_ptr)
    return set_error(HDD_ERR_INVALID, "hdd_shard_pattern_fill: null argument");
  if (sh->host_only) return set_error(HDD_ERR_INVALID, "hdd_shard_pattern_fill: host-only shard (created without a context)");
  hdd_mesh m;
  hdd_shard_mesh(sh, &m);
  int64_t nnz = 0;
  int rc = hdd_pattern_elem_ptr_device(ctx, &m, sh->gi.nb, d_elem_ptr, &nnz, stream);
  if (rc) return rc;
  if (nnz != sh->nnz) return set_error(HDD_ERR_INVALID, "hdd_shard_pattern_fill: nnz mismatch (internal)");
  rc = hdd_pattern_fill_device(ctx, &m, sh->gi.nb, sh->d_gid, d_elem_ptr, d_row_ptr, d_col, stream);
  if (rc) return rc;
  const hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
  return e == hipSuccess ? HDD_OK : hip_fail(e, "hdd_shard_pattern_fill: synchronize");
}
