// vmem_asm.h -- the vector-memory operations the kernels issue BY HAND, one copy each: LDS-DMA requests, 16-byte loads and stores
// the compiler does not count, the s_waitcnt vmcnt(n) statements that cover them.
//
// Why inline assembly at all: issued through the builtin, the compiler knows that memory -> LDS traffic is outstanding and puts
// s_waitcnt vmcnt(0) in front of EVERY LDS access that follows -- it cannot tell the buffers apart -- so a wave sits out the whole
// latency of the tiles it has just requested, each iteration; a counted load, store or returning atomic likewise makes it wait for
// everything older where the value is used.  In inline assembly the compiler does not know that anything is outstanding.  The
// price: EVERY wait on this traffic is counted by hand against an issue-order table that stands in the kernel that uses it (which
// operations a wave issues inside one tile, in which order, and what may still be outstanding at each wait).  A kernel that uses
// this header has no compiler-counted vector-memory operation in flight wherever it waits by hand.
//
// Three wait-state rules.  The compiler's hazard recogniser does not look into inline assembly, so each statement carries its own;
// each was found on the hardware, and tools/asm_hazards.py checks all three in the generated code:
//   1. s_nop 4 in front of every vector-memory instruction that takes a SCALAR base.  The register may have been written by a VALU
//      instruction just in front of the statement (v_readlane of a spilled SGPR, v_readfirstlane), and the ISA asks for five wait
//      states between such a write and a vector-memory instruction that reads it.  Without it: dgrad_r.hip, which has SGPR spills,
//      sent a request with a stale base -- a memory access fault at M = 4 097, none at M = 1 or 33 (the hazard depends on what the
//      allocator put in front of the statement).
//   2. s_nop 1 behind every 16-byte store.  A store of more than 8 bytes reads its data registers for a few cycles after issue.
//      Without it: in dgrad_t.hip the next VALU write to the data registers changed what lanes 8-15 / 24-31 of each half stored
//      (they stored the NEXT store's values).
//   3. a wait state between the scalar write of M0 and the LDS-DMA request that reads it (the ISA asks for one).  In the
//      scalar-base requests rule 1's s_nop 4 stands there; the vector-address form has its own s_nop 0.
#pragma once
#include "common.h"

DEV uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p; }

// One LDS-DMA request (global_load_lds_dwordx4): lane L's 16 bytes at (wave-uniform sbase + voff) land at LDS byte address
// lds_base + 16 L.  HALF: only lanes 0..31 take part (512 bytes) -- the upper half of EXEC is cleared around the request inside the
// one statement (EXEC is full wherever this is called).
template <bool HALF>
DEV void dma_part(const void* sbase, uint32_t voff, uint32_t lds_base) {
  if constexpr (!HALF) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_base), "v"(voff), "s"(sbase) : "memory", "m0");
  } else {
    uint32_t saved;
    asm volatile("s_mov_b32 m0, %1\n\ts_mov_b32 %0, exec_hi\n\ts_mov_b32 exec_hi, 0\n\ts_nop 4\n\tglobal_load_lds_dwordx4 %2, %3\n\ts_mov_b32 exec_hi, %0"
                 : "=&s"(saved)
                 : "s"(lds_base), "v"(voff), "s"(sbase)
                 : "memory", "m0");
  }
}
// ... with a per-lane address `g` (fcln.hip).  No scalar base, so rule 1 does not apply and the statement keeps rule 3's own
// single wait state.
DEV void dma16(const void* g, uint32_t lds_base) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds_base), "v"(g) : "memory", "m0");
}

// fragment load / store the compiler does not count: 16 bytes at sbase + voff + OFF
template <int OFF>
DEV void ldg4_uncounted(f32x4& dst, const void* sbase, uint32_t voff) {
  asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(sbase), "n"(OFF) : "memory");
}
// ... into the AGPR half of the register file (A operands of MFMAs, which read them there)
template <int OFF>
DEV void ldg4_uncounted_a(f32x4& dst, const void* sbase, uint32_t voff) {
  asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2 offset:%3" : "=a"(dst) : "v"(voff), "s"(sbase), "n"(OFF) : "memory");
}
template <int OFF>
DEV void stg4_uncounted(void* sbase, uint32_t voff, f32x4 v) {
  asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 offset:%3\n\ts_nop 1" ::"v"(voff), "v"(v), "s"(sbase), "n"(OFF) : "memory");
}

// Wait until at most KEEP of this wave's vector-memory operations are outstanding.  The registers the wait is for are operands, so
// that no use of them is scheduled in front of it and none of them is given to another value before it (an asm statement takes at
// most 30 operands: sixteen quads per call).
template <int KEEP>
DEV void wait_vm(f32x4 (&r)[4]) {
  asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]) : [n] "n"(KEEP) : "memory");
}
template <int KEEP>
DEV void wait_vm_v16(f32x4* r) {
  asm volatile("s_waitcnt vmcnt(%[n])"
               : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]), "+v"(r[8]), "+v"(r[9]),
                 "+v"(r[10]), "+v"(r[11]), "+v"(r[12]), "+v"(r[13]), "+v"(r[14]), "+v"(r[15])
               : [n] "n"(KEEP)
               : "memory");
}
template <int KEEP>
DEV void wait_vm_a16(f32x4* r) {
  asm volatile("s_waitcnt vmcnt(%[n])"
               : "+a"(r[0]), "+a"(r[1]), "+a"(r[2]), "+a"(r[3]), "+a"(r[4]), "+a"(r[5]), "+a"(r[6]), "+a"(r[7]), "+a"(r[8]), "+a"(r[9]),
                 "+a"(r[10]), "+a"(r[11]), "+a"(r[12]), "+a"(r[13]), "+a"(r[14]), "+a"(r[15])
               : [n] "n"(KEEP)
               : "memory");
}
template <int KEEP>
DEV void wait_vm_v2(f32x4& r0, f32x4& r1) {
  asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(r0), "+v"(r1) : [n] "n"(KEEP) : "memory");
}
template <int KEEP>
DEV void wait_vm_v3(f32x4& r0, f32x4& r1, f32x4& r2) {
  asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(r0), "+v"(r1), "+v"(r2) : [n] "n"(KEEP) : "memory");
}
template <int KEEP>
DEV void wait_vm1(int& r) {
  asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(r) : [n] "n"(KEEP) : "memory");
}
// ... for a value nobody will read: `r` is an input only, which keeps its register occupied up to the wait and gives the compiler no
// new value to copy it into (as an in-out operand the last tile's ticket was moved to another register in front of the wait)
template <int KEEP>
DEV void retire_vm1(int r) {
  asm volatile("s_waitcnt vmcnt(%[n])" ::"v"(r), [n] "n"(KEEP) : "memory");
}

// ---- LDS reads the compiler does not count (lstm16x.hip) ---------------------------------------------------------------------
// The same bargain on the other counter.  A plain C++ LDS load under register pressure is sunk to the MFMA that consumes it and
// waited for there with lgkmcnt(0): the wave sits out the LDS round trip AND whatever younger read it had in flight.  A volatile
// asm read stays where it is written, and the wait that covers it is written by hand as well: the LDS answers a wave's requests
// in order, so `s_waitcnt lgkmcnt(KEEP)` with KEEP = the number of LDS instructions issued behind the wanted one lets exactly
// those stay in flight.  The registers waited for are in-out operands of the wait (no use of them moves in front of it, none is
// copied or given away before it); KEEP comes from the issue-order table in the kernel.  Two rules beyond vmcnt's:
//   * arithmetic (MFMAs included) is scheduled ACROSS asm statements, so a wait + request group stands between two
//     __builtin_amdgcn_sched_barrier(0), one on EACH side: with a fence behind the group only, the MFMAs in front of it slid
//     down behind it and the wait came 1-2 MFMAs after its request;
//   * compiler-counted LDS instructions may share the loop only where no hand-counted wait has them among the instructions it
//     leaves in flight (the compiler pairs ds_write_b32 into ds_write2_b32 as it likes: their number is not the source's).
template <int OFF>
DEV void lds_read4_uncounted(f32x4v& dst, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
template <int KEEP>
DEV void wait_lds(f32x4v& r0) {
  asm volatile("s_waitcnt lgkmcnt(%[n])" : "+v"(r0) : [n] "n"(KEEP) : "memory");
}
template <int KEEP>
DEV void wait_lds(f32x4v& r0, f32x4v& r1) {
  asm volatile("s_waitcnt lgkmcnt(%[n])" : "+v"(r0), "+v"(r1) : [n] "n"(KEEP) : "memory");
}
template <int KEEP>
DEV void wait_lds(f32x4v& r0, f32x4v& r1, f32x4v& r2) {
  asm volatile("s_waitcnt lgkmcnt(%[n])" : "+v"(r0), "+v"(r1), "+v"(r2) : [n] "n"(KEEP) : "memory");
}

// ---- tile tickets of the persistent kernels built on the operations above (dgrad_t.hip, dgrad_r.hip, gemm_t.hip) -----------------
// A workgroup takes 32-token tiles until none is left; the rows of tile i + 1 are requested while tile i multiplies, so the ticket
// of tile i + 2 must be on its way by then.  Thread 0 asks for it with an UNCOUNTED returning atomic right behind the barrier of
// tile i (a counted one would make the compiler wait for everything older, stores included, where the ticket is published),
// keeps the answer in `ticket_ahead`, and publishes it through LDS in front of the barrier of tile i + 1.  The atomic is the oldest
// operation of its tile in the kernel's issue-order table, so any wait of that tile that names `ticket_ahead` covers it:
//   * a tile with a successor ends with wait<KEEP>(): the next tile's rows are in, the ticket with them;
//   * a workgroup's last tile calls retire<KEEP>() in front of its own final stores, KEEP = the previous tile's stores (the only
//     younger operations then): the register stays the ticket's until the atomic has returned, and nothing of it is in flight in
//     whatever follows the loop.  The atomic is a tile old there, so the wait costs nothing.
// queue == nullptr (option "deterministic"): the static order blockIdx.x, + gridDim.x, ..., computed by every wave itself; no
// atomic is issued and the waits name a register nothing writes.
// (common.h's TileTickets is the GEMM engine's mechanism: compiler-counted atomics, one tile ahead.)
struct TicketLoop {
  int ticket_ahead;    // thread 0: the ticket AFTER the next one, requested a tile ago (the first member on purpose: the only one
                       // a tile loop carries; behind the others the kernels' loops came out with their copies in another order)
  int* s_next;         // [2] in LDS: the tile after the current one, per buffer parity
  unsigned* queue;
  int ntiles;
  bool dyn;            // queue != nullptr, wave-uniform (a kernel argument)
  int base;            // added to a ticket where it is published: 0, or the grid where the first tiles are not drawn (StaticFirst)

  // Prologue: thread 0 takes the first two tickets (counted: nothing hand-issued is in flight yet).  The caller may stage what it
  // likes behind it; first_tile() comes after the caller's barrier.
  DEV TicketLoop(int* s_next_, unsigned* queue_, int ntiles_) : ticket_ahead(0), s_next(s_next_), queue(queue_), ntiles(ntiles_), dyn(queue_ != nullptr), base(0) {
    if (dyn) {
      if (threadIdx.x == 0) {
        s_next[0] = (int)atomicAdd(queue, 1u);
        ticket_ahead = (int)atomicAdd(queue, 1u);
      }
    } else if (threadIdx.x == 0) {
      s_next[0] = (int)blockIdx.x;
    }
  }
  // ... for a kernel whose tiles are long and whose grid is the chip (attn_block2.hip: a sequence is ~90 us): a workgroup's FIRST
  // tile is its own number, the counter hands out tiles gridDim.x, gridDim.x + 1, ...  Drawn, the first tickets of a launch are
  // two atomics per workgroup on one address in the same microsecond; they are served one after the other, and the last workgroup
  // had its first tile ~30 us after the launch (measured: + 1.06 ms on a 4.0 ms forward of 33 launches with <= 150 workgroups each).
  // The one request left in the prologue is uncounted like the loop's and covered like it: by the first wait of the first tile
  // that names the ticket.
  struct StaticFirst {};
  DEV TicketLoop(int* s_next_, unsigned* queue_, int ntiles_, StaticFirst)
      : ticket_ahead(0), s_next(s_next_), queue(queue_), ntiles(ntiles_), dyn(queue_ != nullptr), base(queue_ != nullptr ? (int)gridDim.x : 0) {
    if (threadIdx.x == 0) {
      s_next[0] = (int)blockIdx.x;
      if (dyn) asm volatile("s_nop 4\n\tglobal_atomic_add %0, %1, %2, %3 sc0" : "=v"(ticket_ahead) : "v"(0u), "v"(1u), "s"(queue) : "memory");
    }
  }
  DEV int first_tile() const { return __builtin_amdgcn_readfirstlane(s_next[0]); }

  // One step of the protocol, at the top of tile `tile` (its rows in buffer `buf`): publish, barrier, read the next tile, ask for
  // the one after it.  A result >= ntiles: `tile` is this workgroup's last.
  DEV int next_tile(int tile, int buf) {
    const int tid = threadIdx.x;
    if (dyn && tid == 0) s_next[buf ^ 1] = ticket_ahead + base;
    __syncthreads();      // every wave's rows of `tile` are in LDS; everyone is through with the other buffer
    const int next = dyn ? __builtin_amdgcn_readfirstlane(s_next[buf ^ 1]) : tile + (int)gridDim.x;
    if (dyn && tid == 0)
      asm volatile("s_nop 4\n\tglobal_atomic_add %0, %1, %2, %3 sc0" : "=v"(ticket_ahead) : "v"(0u), "v"(1u), "s"(queue) : "memory");
    return next;
  }
  // body(HAS_NEXT, HAS_PREV, next) once per tile, from `tile` (< ntiles) in buffer `buf` on: the four combinations are four
  // instantiations, so a body knows at compile time whether it requests rows of `next` into buffer buf ^ 1 and whether a previous
  // tile's stores are pending.  `tile` and `buf` are the caller's: its body reads them.
  template <class Body>
  DEV void run(int& tile, int& buf, Body&& body) {
    bool first = true;
    while (true) {
      const int next = next_tile(tile, buf);
      if (next < ntiles) {
        if (first) body(std::true_type{}, std::false_type{}, next);
        else body(std::true_type{}, std::true_type{}, next);
        first = false;
        tile = next;
        buf ^= 1;
      } else {
        if (first) body(std::false_type{}, std::false_type{}, next);
        else body(std::false_type{}, std::true_type{}, next);
        break;
      }
    }
  }
  // at most KEEP vector-memory operations younger than the ticket atomic are outstanding
  template <int KEEP>
  DEV void wait() {
    wait_vm1<KEEP>(ticket_ahead);
  }
  template <int KEEP>
  DEV void retire() const {      // ... on a workgroup's last tile
    retire_vm1<KEEP>(ticket_ahead);
  }
};
