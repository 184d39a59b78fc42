// Host check of csrc/sched_check.hpp: every link schedule acs_create_csr_scheduled refuses before a
// handle exists, with the exact code and message, and the schedules on the edge of those checks
// that must pass.  tests/test_sched_check_host.py builds this with -fsanitize=address,undefined and
// runs it; exit status 0 and "sched_check: N checks, 0 failed".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sched_check.hpp"

using namespace acs;

static int g_checks = 0, g_failed = 0;

static acs_config config(uint32_t rule, uint32_t policy = ACS_MISSING_SELF) {
    acs_config c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.n_nodes = 3;
    c.n_instances = 1;
    c.topology = ACS_TOPO_CSR;
    c.rule = rule;
    c.missing_policy = policy;
    return c;
}

static CsrCheck run(const acs_config& c, uint32_t period, const std::vector<uint32_t>& avail, bool null_avail = false) {
    CsrCheck r;
    static const uint32_t none = 0;   // (an empty vector's data() may be null: a graph without slots still has an array)
    sched_check(r, c, avail.size(), period, null_avail ? nullptr : avail.empty() ? &none : avail.data());
    return r;
}

static void expect(const char* what, const CsrCheck& r, int code, const char* message) {
    ++g_checks;
    if (r.code == code && r.message == message) return;
    ++g_failed;
    fprintf(stderr, "%s: got (%d, \"%s\"), want (%d, \"%s\")\n", what, r.code, r.message.c_str(), code, message);
}

static void expect_ok(const char* what, const CsrCheck& r) {
    ++g_checks;
    if (r.code == ACS_OK && r.message.empty()) return;
    ++g_failed;
    fprintf(stderr, "%s: got (%d, \"%s\"), want ok\n", what, r.code, r.message.c_str());
}

int main() {
    const acs_config w = config(ACS_RULE_WEIGHTED), wo = config(ACS_RULE_WEIGHTED, ACS_MISSING_OMIT);
    const acs_config ps = config(ACS_RULE_PUSHSUM), po = config(ACS_RULE_PUSHSUM, ACS_MISSING_OMIT);
    const acs_config ph = config(ACS_RULE_PUSHSUM, ACS_MISSING_HOLD);

    // the mask of a slot that is up in every phase
    ++g_checks;
    if (sched_full_mask(1) != 1u || sched_full_mask(5) != 31u || sched_full_mask(31) != 0x7FFFFFFFu ||
        sched_full_mask(32) != 0xFFFFFFFFu) {
        ++g_failed;
        fprintf(stderr, "sched_full_mask\n");
    }

    // period
    expect("period 0", run(w, 0, {1, 1}), ACS_EINVAL, "link schedule: period 0 outside 1..32");
    expect("period 33", run(w, 33, {1, 1}), ACS_EINVAL, "link schedule: period 33 outside 1..32");
    expect("period 2^32 - 1", run(ph, 0xFFFFFFFFu, {1}), ACS_EINVAL, "link schedule: period 4294967295 outside 1..32");
    expect_ok("period 1", run(w, 1, {1, 0, 1}));
    expect_ok("period 32, bit 31", run(w, 32, {0x80000000u, 0xFFFFFFFFu, 0}));
    // null masks (also with no slot at all: the pointer is an argument error, not an empty array)
    expect("null avail", run(w, 4, {1, 1}, true), ACS_EINVAL, "link schedule: null avail");
    expect("null avail, nnz 0", run(w, 4, {}, true), ACS_EINVAL, "link schedule: null avail");
    expect_ok("nnz 0", run(w, 4, std::vector<uint32_t>()));
    // a bit at a position >= period: the first offending slot is named
    expect("stray bit", run(w, 3, {7, 8, 16}), ACS_EINVAL,
           "link schedule: avail[1] = 0x00000008 has a bit at a position >= period 3");
    expect("stray bit 31", run(po, 31, {0x7FFFFFFFu, 0, 0x80000001u}), ACS_EINVAL,
           "link schedule: avail[2] = 0x80000001 has a bit at a position >= period 31");
    expect("period 1, bit 1", run(wo, 1, {2}), ACS_EINVAL,
           "link schedule: avail[0] = 0x00000002 has a bit at a position >= period 1");
    expect_ok("every bit below the period", run(wo, 3, {7, 0, 5}));
    // dead links are allowed
    expect_ok("all links dead", run(ph, 6, {0, 0, 0, 0}));
    // rules
    const uint32_t others[] = {ACS_RULE_AVERAGE, ACS_RULE_TRIMMED_MEAN, ACS_RULE_MIDPOINT, ACS_RULE_DLPSW_SELECT,
                               ACS_RULE_WMSR};
    for (uint32_t rule : others) {
        char want[128];
        snprintf(want, sizeof want, "link schedules are served for rules WEIGHTED and PUSHSUM (got rule %u)", rule);
        expect("another rule", run(config(rule), 2, {3, 3}), ACS_EUNSUPPORTED, want);
    }
    // PUSHSUM with SELF: only the schedule that never takes a link down
    expect_ok("pushsum SELF, full masks", run(ps, 5, {31, 31, 31}));
    expect_ok("pushsum SELF, full masks, period 32", run(ps, 32, {0xFFFFFFFFu}));
    expect("pushsum SELF, a down phase", run(ps, 5, {31, 15, 31}), ACS_EINVAL,
           "link schedule: PUSHSUM with a slot that is down in some phase (avail[1] = 0x0000000f, period 5) needs "
           "missing_policy = OMIT or HOLD: SELF would put the receiver's own pair in place of the missing message and "
           "create mass");
    expect("pushsum SELF, a dead link", run(ps, 1, {0}), ACS_EINVAL,
           "link schedule: PUSHSUM with a slot that is down in some phase (avail[0] = 0x00000000, period 1) needs "
           "missing_policy = OMIT or HOLD: SELF would put the receiver's own pair in place of the missing message and "
           "create mass");
    expect("pushsum SELF, stray bit first", run(ps, 2, {3, 4}), ACS_EINVAL,
           "link schedule: avail[1] = 0x00000004 has a bit at a position >= period 2");
    expect_ok("pushsum OMIT, down phases", run(po, 5, {1, 15, 0}));
    expect_ok("pushsum HOLD, down phases", run(ph, 5, {1, 15, 0}));
    expect_ok("weighted SELF, down phases", run(w, 5, {1, 15, 0}));

    // a long schedule: every slot is read, none past the end (the sanitizers watch)
    std::vector<uint32_t> big(100000, 0x15u);
    expect_ok("100000 slots", run(ph, 5, big));
    big.back() = 0x20u;
    expect("last slot", run(ph, 5, big), ACS_EINVAL,
           "link schedule: avail[99999] = 0x00000020 has a bit at a position >= period 5");

    fprintf(stderr, "sched_check: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
