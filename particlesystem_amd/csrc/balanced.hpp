// balanced.hpp -- what the plan of the balanced force pass (plan.hip) and the pass itself (force.hip) agree on: the
// wave_pos word and its decoding, the hand-off of a cut task's sums, the waves' pacing
#pragma once

#include "kernels_common.hpp"

namespace psamd {

// A position in the pass's work, the wave_pos word: (task, cost already walked inside the task) as task << 32 | cost.
// Positions order like the (task, stencil step) units they stand for.  k_plan_force writes them, resolve_unit reads them.
__device__ __forceinline__ long long wave_pos_make(int task, int cost) { return ((long long)task << 32) | (long long)cost; }
__device__ __forceinline__ int wave_pos_task(long long pos) { return (int)(pos >> 32); }
__device__ __forceinline__ int wave_pos_cost(long long pos) { return (int)(pos & 0xffffffffll); }

// wave_pos -> (task, stencil step) unit, by the wave that starts (or stops) there.  The stencil step of a position
// (task, cost already walked inside the task) is the number of leading stencil cells the residual covers whole:
// 27 lanes look the cells' populations up, one scan, one ballot.  Every wave of the balanced pass resolves its own two
// boundaries as its first instructions (until round 5 a launch of its own did it, k_resolve_steps: 5.5 us on the step's
// critical path for what a wave does in the shadow of its first loads).  Returns a wave-uniform number.
__device__ __forceinline__ int resolve_unit(const DevParams &P, long long pos, const int *__restrict__ cell_start, const int *__restrict__ task_list)
{
    const int lane = (int)(threadIdx.x & 63);
    const int t = __builtin_amdgcn_readfirstlane(wave_pos_task(pos)), r = __builtin_amdgcn_readfirstlane(wave_pos_cost(pos));
    int k = 0;
    if (r > 0) {
        const int c = __builtin_amdgcn_readfirstlane(task_list[t]) / P.slices;
        int i1, i2, i3, cnt = 0;
        cell_coords(P, c, i1, i2, i3);
        if (lane < STENCIL) {
            const int nc = local_cell(P, i3 + c_stencil[lane][2], i1 + c_stencil[lane][1], i2 + c_stencil[lane][0]);
            if (nc >= 0) cnt = min(cell_start[nc + 1] - cell_start[nc], P.max_per_cell);
        }
        const int cum = wave_incl_scan(cnt);
        k = __popcll(__ballot(lane < STENCIL - 1 && cum <= r));
    }
    return t * STENCIL + k;
}
// Hand-off of a task's partial sums between the wave that walked the first stencil steps and
// the one that continues (balanced force pass).  Follows the guide's inter-workgroup recipe
// (cdna_hip_programming.md, Guideline 16): the payload is stored write-through with agent-scope
// atomic stores, the storing wave drains its stores, ONE lane raises the flag with an agent-scope
// atomic store; the consumer polls that one word relaxed and reads the payload with agent-scope
// atomic loads (they bypass the CU's L1, so no acquire fence is needed).  The flags are zeroed
// with the frame, before the launch.
typedef __attribute__((address_space(1))) unsigned int gu32;
typedef __attribute__((address_space(1))) unsigned long long gu64;

// The flag word carries the stencil step the published sums stand at, so that a task cut in
// three or more pieces hands on correctly at every cut (each consumer waits for ITS step).
__device__ __forceinline__ void handoff_publish(float4 *slot, float ax, float ay, float az, int flag, bool valid, int *ready, int step)
{
    if (valid) {
        gu64 *p = (gu64 *)(unsigned long long *)slot;
        __hip_atomic_store(p, ((unsigned long long)__float_as_uint(ay) << 32) | __float_as_uint(ax), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p + 1, ((unsigned long long)(unsigned)flag << 32) | __float_as_uint(az), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if ((threadIdx.x & 63) == 0) __hip_atomic_store((gu32 *)(unsigned int *)ready, (unsigned)step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// false: the flag never came (bounded spin; the caller raises a sticky error)
__device__ __forceinline__ bool handoff_consume(const float4 *slot, float &ax, float &ay, float &az, int &flag, bool valid, const int *ready, int step)
{
    int ok = 0;
    if ((threadIdx.x & 63) == 0) {
        for (unsigned spins = 0; spins < (1u << 22); spins++) {
            if (__hip_atomic_load((gu32 *)(unsigned int *)ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)step) { ok = 1; break; }
            __builtin_amdgcn_s_sleep(16);
        }
    }
    ok = __builtin_amdgcn_readfirstlane(ok);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");       // compiler-only: the loads below stay below the poll
    if (ok && valid) {
        gu64 *p = (gu64 *)(unsigned long long *)slot;
        const unsigned long long a = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long b = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ax = __uint_as_float((unsigned)a); ay = __uint_as_float((unsigned)(a >> 32));
        az = __uint_as_float((unsigned)b); flag = (int)(unsigned)(b >> 32);
    }
    return ok != 0;
}

// Pacing of the balanced force pass.  All its waves are resident and have the same amount of work, but the SIMD issues
// oldest-first: the seven waves of a SIMD do not advance together, they END one after the other (wave trace, round 4:
// the workgroups dispatched first end at 37 % of the kernel's span, the next at 47 %, ... the last at 92-100 %), and
// for the last 40 % of the launch a SIMD holds fewer than four waves -- at the end a lone one, which cannot cover its
// scalar-load round trips (15 % of the kernel's issue slots idle).  So every wave keeps itself on schedule: at each
// stencil step it compares the share of its work it has done with the share of the pass's expected duration that has
// gone by (the duration of the last such pass, kept in StepState by the planning kernel and the waves themselves) and
// sets its issue priority accordingly -- behind schedule: up, ahead: down.  Waves then advance together and end
// together, whatever their age.  Nothing but issue order changes: same instructions, same results.
struct WavePace {
    unsigned long long t0 = 0;      // when the pass was planned (100 MHz counter)
    float per_tick = 0.f;           // 1 / expected duration of the pass, in ticks; 0: no pacing (no history yet)
    float per_unit = 0.f;           // 1 / the wave's (task, stencil step) units
    int done = 0;                   // units done so far
    int band = 20;                  // how far off schedule (1/1024 of the pass) before the priority goes to an end of its range
    __device__ __forceinline__ void step()
    {
        done++;
        if (per_tick == 0.f) return;
        const float lag = (float)(long long)(__builtin_amdgcn_s_memrealtime() - t0) * per_tick - (float)done * per_unit;
        // (s_setprio is a scalar instruction: it executes whatever EXEC says, so the choice must be a scalar branch --
        // the lag as a wave-uniform integer, in 1/1024 of the pass)
        const int q = __builtin_amdgcn_readfirstlane((int)(lag * 1024.0f));
        if (q > band) __builtin_amdgcn_s_setprio(3);
        else if (q > 0) __builtin_amdgcn_s_setprio(2);
        else if (q > -band) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
    }
};

}  // namespace psamd
