// Host stand-in for csrc/ccp_grid_mg.hpp, for tests/cpp/mgl_host_check.cpp only: what csrc/ccp_grid_mgl.hpp needs to run
// as a host program under a sanitizer, a workgroup being 256 host threads and __syncthreads() a barrier.
// tests/test_mgl_host.py copies the kernel header next to this file, where its #include "ccp_grid_mg.hpp" finds this one.
// kBlock, struct MgLevel and mg_at are NOT restated here: the test cuts their text out of csrc/ccp_common.hpp and
// csrc/ccp_grid_mg.hpp into mgl_host_real.inc, and fails if it cannot find them, so a change to the real definitions
// reaches this program.  Stand-ins of this file's own, to keep in step by hand: Geom (a member of MgLevel that the line
// kernel never reads: empty here) and CgState (the kernel reads `active` alone).
#pragma once
#include <algorithm>
#include <barrier>
#include <cstdio>
#define __global__
#define __shared__ static
#define __restrict__
#define __host__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
struct Idx { unsigned x, y, z; };
inline thread_local Idx threadIdx, blockIdx;
inline std::barrier<> *g_bar;
inline void __syncthreads() { g_bar->arrive_and_wait(); }
using std::min;
namespace ccp {
struct CgState { int active; };
struct Geom {};
#include "mgl_host_real.inc"
}
