// binned_select.hpp — the compiled phase-B kernels (k_bin_gather instantiations, round_binned.hip)
// and the choice of one for a plan state.  Host-only and free of HIP headers, so a host compiler
// builds it (tests/host/binned_select_check.cpp).
//
// The set is written down once, as the predicate gather_compiled() over the kernel's template
// arguments; kGatherTable is every key that satisfies it.  Everything that depends on the set is
// derived from here: the launch table (round_binned.hip), binned_sb_supported, the pass-count clamp
// and the narrow eligibility of binned_build (binned_plan.hip).
#pragma once

#include <stdint.h>

namespace acs {

constexpr uint32_t kBinSB = 256;   // default receivers per phase-B workgroup (engine.hpp)

// compiled (degree, trim) pairs
#define ACS_BINNED_VARIANTS(X) X(16, 5) X(32, 5) X(16, 0) X(32, 0) X(8, 2) X(8, 0)

constexpr bool bin_pair_compiled(uint32_t d, uint32_t t) {
#define X(DD, TT) \
    if (d == DD && t == TT) return true;
    ACS_BINNED_VARIANTS(X)
#undef X
    return false;
}

// receiver blocks other than kBinSB: t = 5 only, d = 16 / 32 at 128 receivers and d = 16 at 512
constexpr bool bin_sb_compiled(uint32_t d, uint32_t t, uint32_t sb) {
    return sb == kBinSB || (t == 5 && ((sb == 128 && (d == 16 || d == 32)) || (sb == 512 && d == 16)));
}

// narrow stage: degrees with a narrow phase B (every compiled trim of them)
constexpr bool bin_narrow_degree(uint32_t d) { return d == 16 || d == 32; }

// most passes a phase B of this flavour is compiled for (clean: neither FAULTY nor FIX)
constexpr uint32_t bin_max_passes(bool f32, bool clean, bool var, uint32_t sb, bool nar) {
    if (var) return 1;                                    // CSR plans: the VAR kernels
    if (nar || sb != kBinSB || !clean) return f32 ? 1 : 2;
    return 4;
}

// template arguments of k_bin_gather, in its parameter order (f32: VT = float)
struct GatherKey {
    uint32_t D, T;
    bool wmsr, faulty, f32;
    uint32_t np;
    bool var, fix;
    uint32_t sb;
    bool nar;
};

constexpr bool operator==(const GatherKey& a, const GatherKey& b) {
    return a.D == b.D && a.T == b.T && a.wmsr == b.wmsr && a.faulty == b.faulty && a.f32 == b.f32 && a.np == b.np &&
           a.var == b.var && a.fix == b.fix && a.sb == b.sb && a.nar == b.nar;
}

constexpr bool gather_compiled(const GatherKey& k) {
    const bool clean = !k.faulty && !k.fix;
    if (!bin_pair_compiled(k.D, k.T) || (k.faulty && k.fix)) return false;
    if (k.f32 && (k.var || k.nar)) return false;   // CSR and narrow plans: fp64
    // other receiver blocks: clean sort-based rules other than W-MSR
    if (k.sb != kBinSB && (!clean || k.var || k.wmsr || k.nar || !bin_sb_compiled(k.D, k.T, k.sb))) return false;
    if (k.nar && (!clean || k.var || !bin_narrow_degree(k.D))) return false;
    return k.np >= 1 && k.np <= bin_max_passes(k.f32, clean, k.var, k.sb, k.nar);
}

constexpr uint32_t kGatherVariants = 229;
struct GatherTable {
    GatherKey row[kGatherVariants];
    uint32_t n;   // keys that satisfy gather_compiled (== kGatherVariants, asserted below)
};

constexpr GatherTable make_gather_table() {
    constexpr uint32_t pairs[][2] = {
#define X(DD, TT) {DD, TT},
        ACS_BINNED_VARIANTS(X)
#undef X
    };
    constexpr uint32_t sbs[] = {kBinSB, 128, 512};
    GatherTable t{};
    for (const auto& pr : pairs)
        for (int f32 = 0; f32 < 2; ++f32)
            for (uint32_t sb : sbs)
                for (int nar = 0; nar < 2; ++nar)
                    for (int var = 0; var < 2; ++var)
                        for (int kind = 0; kind < 3; ++kind)   // clean, FAULTY, FIX
                            for (int w = 0; w < 2; ++w)
                                for (uint32_t np = 1; np <= 4; ++np) {
                                    const GatherKey k{pr[0],    pr[1], w != 0,    kind == 1, f32 != 0,
                                                      np,       var != 0, kind == 2, sb,     nar != 0};
                                    if (!gather_compiled(k)) continue;
                                    if (t.n < kGatherVariants) t.row[t.n] = k;
                                    ++t.n;
                                }
    return t;
}
inline constexpr GatherTable kGatherTable = make_gather_table();
static_assert(kGatherTable.n == kGatherVariants, "kGatherVariants must count the compiled k_bin_gather set");

// ---- selection
// The facts of one launch_round_binned call that decide its phase-B kernel.
struct GatherFacts {
    uint32_t D, trim, rule;   // plan degree, RoundArgs::trim / rule (0 AVERAGE, 4 W-MSR, else sort-based)
    bool f32;
    bool clean;               // no slot-dependent decision
    bool status;              // RoundArgs::status is set (a fault schedule)
    bool var;                 // BinnedPlan::var
    uint32_t split, SB;       // BinnedPlan::split / SB
    bool narrow;              // BinnedPlan::narrow (with its nhdr)
    bool fix;                 // the plan has a fix-up list
    uint32_t phases, sel_n;   // the call's phases and SrcSel::n
    bool omit;                // MsgParams::omit
};

enum class GatherErr : uint8_t { kNone, kNotSupported, kInvalidValue };   // hipErrorNotSupported / InvalidValue

struct GatherChoice {
    GatherErr err;
    uint32_t row;    // index into kGatherTable (err == kNone)
    bool nar, fixp;  // the round runs narrow / applies the fix-up list before phase B
};

inline GatherChoice select_gather(const GatherFacts& f) {
    GatherChoice c{GatherErr::kNone, 0, false, false};
    // narrow plans: clean whole rounds only (the chunked partitioned sequence never builds one)
    c.nar = f.narrow && f.clean && !f.var && f.sel_n == 0 && f.SB == kBinSB;
    if (f.narrow && !c.nar) return {GatherErr::kInvalidValue, 0, false, false};
    if (f.SB != kBinSB && (!f.clean || f.var)) return {GatherErr::kInvalidValue, 0, false, false};
    // fault fix-up on whole rounds; chunked partitioned rounds keep the tagged senders
    c.fixp = !f.clean && f.status && f.fix && f.phases == 7 && f.sel_n == 0 && !f.omit;
    GatherKey k{f.D, f.trim, f.rule == 4, !f.clean && !c.fixp, f.f32, 1, f.var, c.fixp, f.SB, c.nar};
    if (c.nar)
        k.np = f.split;
    else if (f.SB != kBinSB) {
        if (f.rule == 0) c.err = GatherErr::kNotSupported;   // (W-MSR: no such row)
        k.np = f.f32 ? 1 : f.split;                          // fp32: one pass, as at kBinSB
    } else if (f.clean)
        k.np = f.var ? 1 : f.split;
    else   // slot-dependent: fp64 in two passes where the plan has two, one otherwise
        k.np = !f.f32 && !f.var && f.split == 2 ? 2 : 1;
    if (c.err == GatherErr::kNone) {
        c.err = GatherErr::kNotSupported;
        for (uint32_t i = 0; i < kGatherVariants; ++i)
            if (kGatherTable.row[i] == k) {
                c.err = GatherErr::kNone;
                c.row = i;
                break;
            }
    }
    return c;
}

// receiver blocks a clean plan of (d, t, rule) can take: kBinSB always, others where both value
// types have the one-pass kernel
inline bool binned_sb_supported(uint32_t d, uint32_t t, uint32_t rule, uint32_t sb, bool clean_fast) {
    if (sb == kBinSB) return true;
    if (!clean_fast) return false;
    GatherFacts f{d, t, rule, false, true, false, false, 1, sb, false, false, 7, 0, false};
    if (select_gather(f).err != GatherErr::kNone) return false;
    f.f32 = true;
    return select_gather(f).err == GatherErr::kNone;
}

}  // namespace acs
