// neurecon_amd — host pieces shared by nr_neus_render, nr_volsdf_render and nr_unisurf_render.
#pragma once
#include "nr_common.h"
#include "nr_mlp.h"

namespace nr {

// the dynamic-LDS limit of one workgroup on the current device
inline int lds_limit(size_t& bytes) {
  int dev = 0, lds_max = 65536;
  NR_HIP_CHECK(hipGetDevice(&dev));
  NR_HIP_CHECK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  bytes = (size_t)lds_max;
  return NR_OK;
}

// fn(ray0, R) over [0, n) in chunks of at most Rc rays; stops at the first non-zero status
template <class Fn>
int for_chunks(int64_t n, int64_t Rc, Fn fn) {
  for (int64_t r0 = 0; r0 < n; r0 += Rc)
    if (int rc = fn(r0, (int)(n - r0 < Rc ? n - r0 : Rc))) return rc;
  return NR_OK;
}

template <class A>
constexpr bool sample_only_of(const A& a) { return a.sample_only != 0; }
constexpr bool sample_only_of(const NrVolsdfArgs&) { return false; }  // VolSDF has no sample pass
template <class A>
const float* d_all_out_of(const A& a) { return a.d_all_out; }
inline const float* d_all_out_of(const NrVolsdfArgs&) { return nullptr; }

// The clauses every render checks first, and the calc_normal clause that each render checks after its own
// null-argument clauses (kept apart so that the first failing clause of an argument block stays the same).
// `name` is the entry point, e.g. "nr_neus_render".
template <class A>
int check_render_common(const char* name, const A* a) {
  const std::string n(name);
  NR_REQUIRE(a, NR_ERR_ARG, n + ": null args");
  int rc = check_sdf_desc(a->sdf);
  if (rc) return rc;
  if ((rc = check_rad_desc(a->rad))) return rc;
  // an empty shard (multi-GPU ray sharding) may pass null ray / output pointers; the sample pass
  // writes d_all_out alone
  NR_REQUIRE(a->n_rays <= 0 || (a->rays_o && a->rays_d && (sample_only_of(*a) ? d_all_out_of(*a) != nullptr
                                                                               : (a->rgb && a->depth && a->acc))),
             NR_ERR_ARG, n + ": null ray or output pointer");
  return NR_OK;
}
template <class A>
int check_render_normals(const char* name, const A* a) {
  NR_REQUIRE(a->n_rays <= 0 || sample_only_of(*a) || !a->calc_normal || a->normals, NR_ERR_ARG,
             std::string(name) + ": calc_normal needs normals output");
  return NR_OK;
}

}  // namespace nr
