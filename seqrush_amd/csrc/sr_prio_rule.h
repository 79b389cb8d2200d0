// sr_prio_rule.h -- issue priority of the tile code of co-resident workgroups of the blocked kernel (sr_align_blk.inc;
// host twin sr_tile_prio_role_host in sr_twins.cpp, which tests/test_prio_rule_host.py checks), shared like sr_mirror_rule.h.
// DESIGN.md section 4.1.
//
// A SIMD holds one wave of each workgroup resident on its CU, and VALU issue is arbitrated by priority, then by age.  The
// workgroups are persistent, so with every wave at priority 0 the age order -- the order in which the workgroups were
// dispatched to the CU -- would decide who is served first for the whole launch.  The rule hands the levels round: a
// workgroup's rank among the workgroups of its CU (its arrival count in SrAlignArgs::cu_arrivals modulo the workgroups
// per CU) plus the epoch (the 100 MHz real-time counter >> SR_PRIO_EPOCH_SHIFT, the same value on every CU) picks one
// of the s_setprio levels 0 .. 3 for the tile code of a pass.  Priority cannot change a result.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SR_PRIO_HD __host__ __device__
#else
#define SR_PRIO_HD
#endif

#define SR_PRIO_EPOCH_SHIFT 11     // 2^11 ticks of 10 ns = 20 us, a quarter of a pass of a loaded CU (measured against 13 and 15)
// SrAlignArgs::cu_arrivals: one word per (XCC, SE, SH, CU) as the hardware ids number them: 4 + 3 + 1 + 4 bits
#define SR_PRIO_TABLE 4096
SR_PRIO_HD inline unsigned sr_prio_table_index(unsigned xcc_id, unsigned se_sh_cu) { return ((xcc_id & 15u) << 8 | (se_sh_cu & 255u)) & (SR_PRIO_TABLE - 1u); }

// position (rank + epoch) mod wg_per_cu, spread over the four levels: 4 per CU hold four distinct levels at any time and
// every workgroup holds every level once in four epochs; 2 per CU hold {0, 2}; more than 4 share levels evenly.
// wg_per_cu <= 1: nothing to arbitrate, always 0 (the feature is off).
SR_PRIO_HD inline int sr_tile_prio_role(unsigned rank, unsigned epoch, unsigned wg_per_cu) {
    if (wg_per_cu <= 1u) return 0;
    const unsigned pos = (rank % wg_per_cu + epoch % wg_per_cu) % wg_per_cu;
    return (int)(pos * 4u / wg_per_cu);
}
