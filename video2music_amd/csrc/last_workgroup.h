// The in-launch hand-off of the training reductions: every workgroup leaves its partial result in its own part of a workspace `ws`,
// and the one that finishes last adds the parts in workgroup order (norm_bwd.hip, chord_loss.hip, reg_loss.hip).  DESIGN.md, "The
// last-workgroup sum", has the scheme, its cost and what it was measured at; the contract and the order of the steps are here.
#pragma once
#include "amt_common.h"

// ws[0] is the ticket counter, at the head of a block of 16 bytes so that the parts behind it stay 16-byte aligned; workgroup b's part
// starts at ws + WS_HEAD + b * (its size).  The counter must be zero when the launch starts: last_workgroup_reset, every call.
constexpr int WS_HEAD = 4;

// Every thread of the workgroup calls this after its last store to the workgroup's part of ws (plain stores), with nb the launch's
// workgroup count.  Returns, the same value in every thread, whether this workgroup drew the last of the nb tickets; where it did, every
// thread may read all nb parts with plain vector loads.  s_flag is a word of an LDS array the kernel already has and has finished
// reading (a second __shared__ object for it is what the kernels avoid); it is overwritten.  Step by step:
//   s_waitcnt vmcnt(0) in every wave, then the barrier: all of the workgroup's stores have left their waves before thread 0 releases;
//   thread 0's agent-scope release fence writes them back to where every other XCD's workgroups read, and the second wait keeps the
//     ticket add behind that write-back whatever the compiler makes of the fence's own wait: fence, wait, add, in this order;
//   the add itself is relaxed: the fences carry the ordering, once per workgroup;
//   the last arriver's acquire fence drops what its caches hold of the other parts, before the barrier that lets its waves read them.
// The parts must be read through pointers the compiler cannot prove read-only for the kernel's lifetime (no const __restrict__ alias
// of ws): a load it moved to the scalar path, or above the barrier, would miss the acquire.
__device__ __forceinline__ bool last_workgroup(float* ws, unsigned nb, unsigned* s_flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned ticket = __hip_atomic_fetch_add(reinterpret_cast<unsigned*>(ws), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = ticket == nb - 1;
        *s_flag = last;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(*s_flag) != 0;
}

// The launcher's side: ws given and 16-byte aligned, its head zeroed on the stream ahead of the launch.  `entry` names the entry point
// in the message; the status is the library's (0 ok, <0 bad argument, >0 hipError_t).
static inline int32_t last_workgroup_reset(float* ws, const char* entry, hipStream_t stream) {
    AMT_CHECK_ARG(ws, "%s: null pointer", entry);
    AMT_CHECK_ARG(((uintptr_t)ws & 15) == 0, "%s: ws must be 16-byte aligned", entry);
    AMT_HIP(hipMemsetAsync(ws, 0, WS_HEAD * sizeof(float), stream));
    return 0;
}
