// Translation unit of the tied-states plan (namp_states.h): namp_states_plan of include/namp.h.
// Host code only validates and enqueues one launch on the caller's stream.
#include "../../include/namp.h"
#include "namp_states.h"

#include <cstdio>
#include <mutex>

__attribute__((visibility("hidden"))) int namp_internal_fail(int code, const char* msg);

namespace {

int sfail(int code, const char* fmt, long a = 0, long b = 0, long c = 0, long d = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b, c, d);
  return namp_internal_fail(code, buf);
}

std::once_flag g_states_once;
hipError_t g_states_err = hipSuccess;
void set_states_attrs() {
  auto set = [](const void* f) {
    hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)STATES_PLAN_LDS(8192));
    if (e != hipSuccess) g_states_err = e;
  };
  set((const void*)states_plan_kernel<1>);
  set((const void*)states_plan_kernel<2>);
  set((const void*)states_plan_kernel<4>);
  set((const void*)states_plan_kernel<8>);
}

}  // namespace

extern "C" int namp_states_plan(const int32_t* E_idx, const int32_t* order0, const int32_t* rank0, const float* weights,
                                int32_t* E_flat, int32_t* order, int32_t* rank, int32_t* group_first, int32_t* group_last, float* sym_w,
                                int32_t* work_n, int32_t* level, int32_t* work, int32_t* level_off, int32_t* n_levels,
                                int32_t* close, int32_t* close_off, int B_dec, int M, int N, int K, void* stream) {
  if (!E_idx || !order0 || !rank0 || !weights || !E_flat || !order || !rank || !group_first || !group_last || !sym_w || !work_n ||
      !level || !work || !level_off || !n_levels || !close || !close_off)
    return sfail(NAMP_EINVAL, "namp_states_plan: null pointer argument");
  if (B_dec < 1 || M < 1 || N < 1 || K < 1 || K > NAMP_MAX_K || N > 8192 || (long)M * N > 16000 || (long)B_dec * M * N >= (1L << 28))
    return sfail(NAMP_EINVAL, "namp_states_plan: bad dims B_dec=%ld M=%ld N=%ld K=%ld (N <= 8192, M * N <= 16000)", B_dec, M, N, K);
  std::call_once(g_states_once, set_states_attrs);
  if (g_states_err != hipSuccess) return sfail(NAMP_ELAUNCH, "namp_states_plan: hipFuncSetAttribute failed");
  const StatesPlan p = {E_idx, order0, rank0, weights, E_flat, order, rank, group_first, group_last, sym_w, work_n, level, work,
                        level_off, n_levels, close, close_off, B_dec, M, N, K};
  const long fill = (long)M * N * (K > B_dec ? K : B_dec);
  long blocks = (fill + 4095) / 4096;
  blocks = blocks < 1 ? 1 : (blocks > 64 ? 64 : blocks);
  const dim3 grid((unsigned)(1 + blocks)), block(1024);
  const size_t lds = STATES_PLAN_LDS(N);
  hipStream_t s = (hipStream_t)stream;
  const int mk = M * K;
  if (mk <= 64) hipLaunchKernelGGL(states_plan_kernel<1>, grid, block, lds, s, p);
  else if (mk <= 128) hipLaunchKernelGGL(states_plan_kernel<2>, grid, block, lds, s, p);
  else if (mk <= 256) hipLaunchKernelGGL(states_plan_kernel<4>, grid, block, lds, s, p);
  else hipLaunchKernelGGL(states_plan_kernel<8>, grid, block, lds, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return sfail(NAMP_ELAUNCH, "namp_states_plan: launch failed");
  return NAMP_OK;
}
