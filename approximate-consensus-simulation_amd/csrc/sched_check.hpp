// sched_check.hpp — host checks of a link schedule ("Link schedules"), before any
// handle or device memory exists (create.hip, create_impl), after the checks of csr_check.hpp.
// Host-only, no HIP header, in the manner of csr_check.hpp: tests/host/sched_check.cpp feeds it
// every rejected input on the CPU.
#pragma once

#include "csr_check.hpp"

static_assert(ACS_SCHEDULE_MAX_PERIOD == 32, "one uint32 mask per slot");

namespace acs {

// every bit of a full mask: the slot is up in every phase (period 32: all 32 bits, no 1u << 32)
inline uint32_t sched_full_mask(uint32_t period) { return period >= 32 ? 0xFFFFFFFFu : (1u << period) - 1u; }

// A schedule is a period P in 1..32 and one mask per CSR slot: bit p < P set = the slot is up in
// every round r with r mod P == p; bits at positions >= P must be zero; a zero mask (a dead link)
// is allowed.  Served for rules WEIGHTED and PUSHSUM.  PUSHSUM with missing_policy = SELF needs
// every slot up in every phase, for the reason loss needs OMIT or HOLD: SELF would put the
// receiver's own pair in place of the missing message and create mass.
// split (acs_create_csr_split, "Push-sum with per-round splitting"): senders pay nothing out on a
// down link, so nothing is missing there and SELF takes any mask.
inline int sched_check(CsrCheck& r, const acs_config& c, uint64_t nnz, uint32_t period, const uint32_t* avail,
                       bool split = false) {
    if (c.rule != ACS_RULE_WEIGHTED && c.rule != ACS_RULE_PUSHSUM)
        return r.fail(ACS_EUNSUPPORTED, "link schedules are served for rules WEIGHTED and PUSHSUM (got rule %u)", c.rule);
    if (period < 1 || period > ACS_SCHEDULE_MAX_PERIOD)
        return r.fail(ACS_EINVAL, "link schedule: period %u outside 1..%u", period, (unsigned)ACS_SCHEDULE_MAX_PERIOD);
    if (!avail) return r.fail(ACS_EINVAL, "link schedule: null avail");
    const uint32_t full = sched_full_mask(period);
    for (uint64_t e = 0; e < nnz; ++e)
        if (avail[e] & ~full)
            return r.fail(ACS_EINVAL, "link schedule: avail[%llu] = 0x%08x has a bit at a position >= period %u",
                          (unsigned long long)e, avail[e], period);
    if (c.rule == ACS_RULE_PUSHSUM && c.missing_policy == ACS_MISSING_SELF && !split)
        for (uint64_t e = 0; e < nnz; ++e)
            if (avail[e] != full)
                return r.fail(ACS_EINVAL, "link schedule: PUSHSUM with a slot that is down in some phase (avail[%llu] = 0x%08x, "
                                          "period %u) needs missing_policy = OMIT or HOLD: SELF would put the receiver's own "
                                          "pair in place of the missing message and create mass",
                              (unsigned long long)e, avail[e], period);
    return ACS_OK;
}

}  // namespace acs
