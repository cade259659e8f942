// dune-hdd_amd/csrc/kernels/rccl_api.hip
//
// RCCL, resolved at run time: in a PyTorch process this is torch's own librccl (already loaded, found
// through the library's rpath), so the process holds one RCCL and one HIP runtime.
#include <dlfcn.h>

#include <type_traits>

#include "shard_internal.hh"

namespace hdd {
namespace shard {

static RcclApi load_rccl()
{
  RcclApi r;
  void* h = nullptr;
  for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"}) {
    h = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
    if (h) break;
  }
  if (!h)
    for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"}) {
      h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (h) break;
    }
  if (!h) {
    const char* e = dlerror();
    r.err = std::string("librccl not found: ") + (e ? e : "");
    return r;
  }
  bool all = true;
  auto sym = [&](auto& fp, const char* name) {
    fp = reinterpret_cast<std::remove_reference_t<decltype(fp)>>(dlsym(h, name));
    if (!fp) {
      all = false;
      r.err += std::string(" missing ") + name;
    }
  };
  sym(r.GetUniqueId, "ncclGetUniqueId");
  sym(r.CommInitRank, "ncclCommInitRank");
  sym(r.CommDestroy, "ncclCommDestroy");
  sym(r.GroupStart, "ncclGroupStart");
  sym(r.GroupEnd, "ncclGroupEnd");
  sym(r.Send, "ncclSend");
  sym(r.Recv, "ncclRecv");
  sym(r.GetErrorString, "ncclGetErrorString");
  r.ok = all;
  return r;
}

const RcclApi& rccl()
{
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] { api = load_rccl(); });
  return api;
}

int nccl_fail(ncclResult_t r, const char* where)
{
  const char* s = rccl().GetErrorString ? rccl().GetErrorString(r) : "?";
  return set_error(HDD_ERR_HIP, std::string(where) + ": RCCL error " + std::to_string(int(r)) + " (" + s + ")");
}

}  // namespace shard
}  // namespace hdd
