// Inter-workgroup hand-off of the read-only reduction kernels: every workgroup leaves ONE record of fp64 partial sums, draws a ticket, and the
// workgroup that draws the last ticket adds the records in a fixed order.  No floating-point atomics, no second launch, no host sync: every
// sum has a fixed order, so the results are bit-reproducible run to run and under HIP-graph replay.
//
// This header is the one place where that protocol is spelled out.  Its users: edge_fast.hpp (forward_tail of every edge_loss.hip forward kernel: per (scale, sample),
// then per launch), edge_loss_kinds.hip (forward_tail: per sample, then per launch), supervised_loss.hip (sup_fwd_kernel: per launch) and norm_act.hip
// (gn_stats_kernel: per sample).  The fixed-order reductions themselves differ per kernel and stay with the kernels.
//
//   writer, the threads that hold a value:   handoff::publish(record + i, v);
//   writer, EVERY thread of the workgroup:   if (!handoff::arrive([&] { return ticket; }, [&] { return workgroups; }, fences, fences, &s_last)) return;
//                                            (= handoff::drain(); then handoff::draw(...) with the same arguments)
//   last arriver:                            v = handoff::read(record_of_workgroup_j + i) for j in the kernel's fixed order
//
// Why each step has the form it has (MI355X, ROCm 7.2):
//   * publish is a RETURNING exchange.  The value comes back only after the store has been performed at the memory side; a plain store, or a
//     no-return atomic, is acknowledged earlier, and the ticket was seen to overtake such a record about once per few thousand workgroups.  The
//     empty asm uses the returned value, so that the exchange keeps its returning form.
//   * arrive drains the vector-memory counter (the exchanges are back) in every wave BEFORE the barrier, so thread 0 draws the ticket only once
//     every record value of the workgroup is at the memory side.
//   * the ticket is an agent-scope relaxed fetch_add: one word per hand-off, zero before the first arrival.
//   * read is an agent-scope relaxed atomic load: performed at the memory side, never served from a compute unit's L1 (the record slots are used again
//     launch after launch, and nothing else in the protocol invalidates that L1).
//   Returning exchanges + agent-scope atomic loads are the form MI355X_MICROARCH.md's visibility table lists as measured-valid.
//
// mte_set_option(MTE_OPT_HANDOFF_FENCES, v) (g_mte_handoff_fences, defined in norm_act.hip; the launchers copy it into a kernel argument, this
// header reads no globals): with v = 1 thread 0 issues an agent-scope RELEASE before it draws the ticket and the last arriver an agent-scope
// ACQUIRE before the records are read, which makes the protocol independent of that table.  Each fence is followed by a wait of its own, fence
// first, then wait, then the ticket, so that the order does not rest on how the fence builtin happens to be lowered.  The two are separate arguments because a
// release also writes back every output line the workgroup stored through its L2: free in the loss kernels, which store nothing but their
// records, but not in GroupNorm's residual-tail statistics pass, which writes its activations on the way and therefore never releases.
#pragma once
#include <hip/hip_runtime.h>

namespace handoff {

__device__ __forceinline__ void publish(double* slot, double v) {
    const unsigned long long before = atomicExch((unsigned long long*)slot, (unsigned long long)__double_as_longlong(v));
    asm volatile("" ::"v"(before));
}

__device__ __forceinline__ double read(const double* slot) { return __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// arrive = drain, then draw.  Both are called by EVERY thread of the workgroup, once its publish calls are issued.  A kernel that has
// workgroup-wide work to place between the barrier and the ticket (forward_tail of edge_fast.hpp reads its image's record count there) calls the two itself.
//
// drain: every wave waits for its exchanges to come back, then the workgroup meets.
__device__ __forceinline__ void drain() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}
// draw: thread 0 draws the ticket.  True in the workgroup that draws the last of `expected()` tickets; every record is then readable.
// ticket_of() -> unsigned*, expected() -> count: callables, evaluated by thread 0 only.
// release / acquire: the fences described above, normally both the kernel's `fences` argument.  s_last: an int of LDS for the broadcast.
// RESET: the last arriver puts the ticket back to 0, so that the buffer holding it can be used again without being cleared.
//
// The callables and the two references are there for code generation only; the result is the same whatever a caller passes.  Written in
// place, the old code read the ticket, the count and `fences` from the kernel arguments inside thread 0's branch.  As by-value parameters
// they are evaluated by every wave before the barrier and stay live to the end of the kernel, and the compiler then gives the edge-loss and
// supervised-loss forward kernels more SGPRs and another instruction order than before the protocol moved here (compile either form with
// -Rpass-analysis=kernel-resource-usage to see it).  A caller keeps the old code only if it passes its kernel-argument members directly, as
// all four do; passing copies held in locals is correct and loses just that.
template <bool RESET = false, typename Ticket, typename Expected, typename Flag>
__device__ __forceinline__ bool draw(Ticket ticket_of, Expected expected, const int& release, const int& acquire, Flag* s_last) {
    if (threadIdx.x == 0) {
        if (release) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
        unsigned* const ticket = ticket_of();
        *s_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)expected() - 1u;
        if constexpr (RESET) {
            if (*s_last) {
                __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (acquire) { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
            }
        } else if (*s_last && acquire) { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
    }
    __syncthreads();
    return *s_last != 0;
}
template <bool RESET = false, typename Ticket, typename Expected, typename Flag>
__device__ __forceinline__ bool arrive(Ticket ticket_of, Expected expected, const int& release, const int& acquire, Flag* s_last) {
    drain();
    return draw<RESET>(ticket_of, expected, release, acquire, s_last);
}

}  // namespace handoff
