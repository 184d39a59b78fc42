// Host check of csrc/binned_select.hpp: the phase-B kernel chosen for every plan state binned_build
// can produce (and a few it cannot, which must be refused), one line per state on stdout;
// tests/test_binned_select_host.py compares the lines with tests/golden/binned_gather_select.txt,
// recorded from the launch ladders this header replaced.  Also: the table lists 229 kernels over
// the six (d, t) pairs, and every one of them is chosen by some reachable state.
#include <cstdio>
#include <cstdlib>

#include "binned_select.hpp"

using namespace acs;

// ---- the enumerated states (shared verbatim with the recording harness of the fixture)
struct State {
    uint32_t D, T, rule;
    bool f32, clean, status, fix, var;
    uint32_t split, SB;
    bool narrow, omit;
    uint32_t sel_n, phases;
    const char* kind;
    bool unreachable;   // no plan reaches this state: it must be refused
};

static void print_state(const State& z) {
    // d t rule type kind var split SB narrow
    printf("%u %u %u %s %s %d %u %u %d: ", z.D, z.T, z.rule, z.f32 ? "f32" : "f64", z.kind, (int)z.var, z.split, z.SB,
           (int)z.narrow);
}

template <typename F>
static void enumerate(F emit) {
    static const uint32_t pairs[6][2] = {{16, 5}, {32, 5}, {16, 0}, {32, 0}, {8, 2}, {8, 0}};
    static const uint32_t rules[3] = {0, 1, 4};   // AVERAGE, sort-based, W-MSR
    static const uint32_t sbs[3] = {128, 256, 512};
    // clean; lossy (slot-dependent, no fault schedule); tagged senders; fix-up list on a whole round,
    // and the same plan where the round keeps the tagged senders (OMIT, or phase B alone)
    struct Kind {
        const char* name;
        bool clean, status, fix, omit;
        uint32_t phases;
    };
    static const Kind kinds[6] = {{"clean", true, false, false, false, 7},  {"lossy", false, false, false, false, 7},
                                  {"tagged", false, true, false, false, 7}, {"fixup", false, true, true, false, 7},
                                  {"fixup+omit", false, true, true, true, 7}, {"fixup/B", false, true, true, false, 4}};
    // ---- reachable states (the invariants binned_build and binned_block_size enforce)
    for (const auto& pr : pairs)
        for (uint32_t rule : rules)
            for (int f32 = 0; f32 < 2; ++f32)
                for (const Kind& k : kinds)
                    for (int var = 0; var < 2; ++var)
                        for (uint32_t split = 1; split <= 4; ++split)
                            for (uint32_t sb : sbs)
                                for (int nar = 0; nar < 2; ++nar) {
                                    const uint32_t D = pr[0], T = pr[1];
                                    if (rule == 0 && T != 0) continue;   // AVERAGE: untrimmed only
                                    if (f32 && var) continue;            // CSR plans: fp64
                                    if (var && split != 1) continue;     // CSR plans: one pass
                                    if (k.status && split > (f32 ? 1u : 2u)) continue;   // fault schedules
                                    if (sb != 256) {   // other receiver blocks: clean, compiled (d, sb) of t = 5
                                        if (!k.clean || var || T != 5 || rule == 4 || rule == 0) continue;
                                        if (!((sb == 128 && (D == 16 || D == 32)) || (sb == 512 && D == 16))) continue;
                                    }
                                    if (nar && (f32 || !k.clean || var || sb != 256 || split > 2 || (D != 16 && D != 32)))
                                        continue;
                                    emit(State{D, T, rule, f32 != 0, k.clean, k.status, k.fix, var != 0, split, sb, nar != 0,
                                               k.omit, 0, k.phases, k.name, false});
                                }
    // ---- states no plan reaches: every one must be refused
    const State refused[] = {
        {16, 5, 1, false, true, false, false, false, 1, 128, true, false, 0, 7, "clean", true},    // narrow, other block
        {32, 5, 1, false, true, false, false, false, 1, 512, false, false, 0, 7, "clean", true},   // 512 receivers at d = 32
        {16, 5, 4, false, true, false, false, false, 1, 128, false, false, 0, 7, "clean", true},   // W-MSR at 128 receivers
        {16, 5, 0, false, true, false, false, false, 1, 128, false, false, 0, 7, "clean", true},   // AVERAGE at 128 receivers
        {16, 0, 1, false, true, false, false, false, 1, 128, false, false, 0, 7, "clean", true},   // t = 0 at 128 receivers
        {8, 2, 1, false, true, false, false, false, 1, 128, false, false, 0, 7, "clean", true},    // d = 8 at 128 receivers
        {16, 5, 1, false, false, true, false, false, 1, 128, false, false, 0, 7, "tagged", true},  // tagged, other block
        {16, 5, 1, false, true, false, false, true, 1, 128, false, false, 0, 7, "clean", true},    // CSR, other block
        {8, 2, 1, false, true, false, false, false, 1, 256, true, false, 0, 7, "clean", true},     // narrow at d = 8
        {32, 5, 1, false, true, false, false, false, 3, 256, true, false, 0, 7, "clean", true},    // narrow in three passes
        {32, 5, 1, false, true, false, false, true, 1, 256, true, false, 0, 7, "clean", true},     // narrow CSR plan
        {32, 5, 1, false, false, true, false, false, 1, 256, true, false, 0, 7, "tagged", true},   // narrow, tagged
        {32, 5, 1, false, true, false, false, false, 2, 256, true, false, 1, 7, "clean", true},    // narrow, chunked round
        {8, 5, 1, false, true, false, false, false, 1, 256, false, false, 0, 7, "clean", true},    // no such (d, t)
        {64, 0, 1, true, true, false, false, false, 1, 256, false, false, 0, 7, "clean", true},    // no such (d, t)
    };
    for (const State& z : refused) emit(z);
}
// ---- end of the enumerated states

static bool chosen[kGatherVariants];
static int bad;

static void emit(const State& z) {
    const GatherFacts f{z.D,   z.T,     z.rule, z.f32,    z.clean, z.status, z.var,
                        z.split, z.SB, z.narrow, z.fix, z.phases, z.sel_n, z.omit};
    const GatherChoice c = select_gather(f);
    print_state(z);
    if (c.err == GatherErr::kNone) {
        const GatherKey& k = kGatherTable.row[c.row];
        chosen[c.row] = true;
        printf("<%u,%u,%d,%d,%s,%u,%d,%d,%u,%d>\n", k.D, k.T, (int)k.wmsr, (int)k.faulty, k.f32 ? "f32" : "f64",
               k.np, (int)k.var, (int)k.fix, k.sb, (int)k.nar);
        // the side results follow the chosen kernel
        if (c.nar != k.nar || c.fixp != k.fix) {
            fprintf(stderr, "side results disagree with row %u\n", c.row);
            ++bad;
        }
    } else {
        printf("%s\n", c.err == GatherErr::kNotSupported ? "NotSupported" : "InvalidValue");
    }
    if (z.unreachable && c.err == GatherErr::kNone) {
        fprintf(stderr, "an unreachable state was not refused\n");
        ++bad;
    }
}

int main() {
    enumerate(emit);
    // the table: 229 distinct kernels over the six pairs, none dead
    static_assert(kGatherVariants == 229, "compiled k_bin_gather set");
    for (uint32_t i = 0; i < kGatherVariants; ++i) {
        const GatherKey& k = kGatherTable.row[i];
        if (!gather_compiled(k) || !bin_pair_compiled(k.D, k.T)) {
            fprintf(stderr, "row %u is not a compiled kernel\n", i);
            ++bad;
        }
        for (uint32_t j = 0; j < i; ++j)
            if (kGatherTable.row[j] == k) {
                fprintf(stderr, "rows %u and %u are equal\n", j, i);
                ++bad;
            }
        if (!chosen[i]) {
            fprintf(stderr, "row %u <%u,%u,%d,%d,%s,%u,%d,%d,%u,%d> is chosen by no reachable state\n", i, k.D, k.T,
                    (int)k.wmsr, (int)k.faulty, k.f32 ? "f32" : "f64", k.np, (int)k.var, (int)k.fix, k.sb, (int)k.nar);
            ++bad;
        }
    }
    fprintf(stderr, "table: %u kernels, %d problems\n", kGatherTable.n, bad);
    return bad ? 1 : 0;
}
