// Translation unit of the base-paired design plan (namp_pairs.h): namp_pairs_plan and namp_pairs_work_lists of include/namp.h.
// Host code only validates and enqueues one launch each on the caller's stream.
#include "../../include/namp.h"
#include "namp_pairs.h"

#include <cstdio>
#include <mutex>

__attribute__((visibility("hidden"))) int namp_internal_fail(int code, const char* msg);

namespace {

int pfail(int code, const char* fmt, long a = 0, long b = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b);
  return namp_internal_fail(code, buf);
}

std::once_flag g_pairs_once;
hipError_t g_pairs_err = hipSuccess;
void set_pairs_attrs() {
  g_pairs_err = hipFuncSetAttribute((const void*)pairs_work_lists_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PAIRS_LISTS_LDS(8192));
}

}  // namespace

extern "C" int namp_pairs_plan(const int32_t* partner, const int32_t* first, const int32_t* order0, const int32_t* rank0, int32_t* order,
                               int32_t* rank, int32_t* group_first, int32_t* group_last, int B_dec, int N, void* stream) {
  if (!partner || !first || !order0 || !rank0 || !order || !rank || !group_first || !group_last)
    return pfail(NAMP_EINVAL, "namp_pairs_plan: null pointer argument");
  if (B_dec < 1 || N < 1 || N > 8192 || (long)B_dec * N >= (1L << 28))
    return pfail(NAMP_EINVAL, "namp_pairs_plan: bad dims B_dec=%ld N=%ld (N <= 8192)", B_dec, N);
  const PairsPlan p = {partner, first, order0, rank0, order, rank, group_first, group_last, B_dec, N};
  hipLaunchKernelGGL(pairs_plan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, p);
  if (hipGetLastError() != hipSuccess) return pfail(NAMP_ELAUNCH, "namp_pairs_plan: launch failed");
  return NAMP_OK;
}

extern "C" int namp_pairs_work_lists(const int32_t* level, const int32_t* group_first, int32_t* work, int32_t* work_n, int32_t* level_off,
                                     int32_t* n_levels, int B_dec, int N, void* stream) {
  if (!level || !group_first || !work || !work_n || !level_off || !n_levels)
    return pfail(NAMP_EINVAL, "namp_pairs_work_lists: null pointer argument");
  if (B_dec < 1 || N < 1 || N > 8192 || (long)B_dec * N >= (1L << 28))
    return pfail(NAMP_EINVAL, "namp_pairs_work_lists: bad dims B_dec=%ld N=%ld (N <= 8192)", B_dec, N);
  std::call_once(g_pairs_once, set_pairs_attrs);
  if (g_pairs_err != hipSuccess) return pfail(NAMP_ELAUNCH, "namp_pairs_work_lists: hipFuncSetAttribute failed");
  hipLaunchKernelGGL(pairs_work_lists_kernel, dim3(1), dim3(1024), PAIRS_LISTS_LDS(N), (hipStream_t)stream, level, group_first, B_dec, N, work,
                     work_n, level_off, n_levels);
  if (hipGetLastError() != hipSuccess) return pfail(NAMP_ELAUNCH, "namp_pairs_work_lists: launch failed");
  return NAMP_OK;
}
