// search.cpp -- the host layer of the exhaustive-search family of the C ABI (include/mimc3_hip.h): mimc3_match_ncc_full, _full_multi,
// _full_planes, _full_dn, _full_any, _full_surf, _full_chip, _full_chip_class, _full_chip_planes, _wide, _wide_class, _wide_planes, _wide_chip, forward-backward (_full_fb, _wide_fb) and the coarse-to-fine searches (_pyramid, _pyramid_dn,
// _pyramid_any, _pyramid_chip), each with its _dev twin.  One shape for all of them: an entry describes its call (SearchCall) and what it accepts
// (SearchRules); search_check makes every refusal, pick_kernel selects the kernel, plane_set points at the planes it reads (building
// them on first use), launch_search is the one place that launches.  The stack's layer adds (stack.cpp) go through the same functions.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include "ctx_internal.h"
#include "sat_kernel.h"
#include "fb_kernel.h"

namespace mimc3 {

bool full_ocw_ok(int32_t ocw) { return ocw == 7 || ocw == 15 || ocw == 16 || ocw == 30 || ocw == 32 || ocw == 40; }
// what the float wide kernel (mimc3_match_ncc_wide beyond R 15) takes
static bool wide_float_takes(int32_t ocw, int32_t R) { return full_ocw_ok(ocw) && R <= wide_max_radius(ocw); }

// the pair's class; that of a pair which is neither 8-bit nor scaled-integer needs its f32 planes: built here on first use (drains the stream)
int pair_class(mimc3_ctx *c, PairClass &cls)
{
    cls = c->u8_ok ? kU8 : kScaledInt;
    if (c->u8_ok || c->u16_ok) return 0;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->fplanes_ok) RC_TRY(build_f32(c));
    cls = c->f32i_ok ? kIntegralF32 : kFloat;
    return 0;
}

// MIMC3_EUNSUPPORTED for a pair of a class beyond `widest` (the f32 planes are only built where the answer needs them)
static int check_class(mimc3_ctx *c, PairClass widest, const std::string &en)
{
    if (widest == kFloat || c->u8_ok) return 0;
    if (widest == kU8) return fail(MIMC3_EUNSUPPORTED, en + ": the pair is not 8-bit (u8 planes only)");
    if (c->u16_ok) return 0;
    if (widest == kScaledInt) return fail(MIMC3_EUNSUPPORTED, en + ": the pair is neither 8-bit nor scaled-integer (u8 or u16 planes only)");
    PairClass cls;
    RC_TRY(pair_class(c, cls));
    if (cls == kFloat)
        return fail(MIMC3_EUNSUPPORTED, en + ": the pair is neither 8-bit, scaled-integer nor integral f32 (pixels x 1 or x 8 integers below 2^20)");
    return 0;
}

// Every refusal the family makes from a call's description, in this order (the first one met decides the code):
//   1. the arguments, MIMC3_EINVAL: a null context, point array or record, N <= 0, candidates that do not go with npeaks, no surfaces
//      where the entry is for them (mimc3_match_ncc_full_surf); npeaks out of range; ocw not one of the six (any_ocw: outside 1..80); R outside 1..15 (wide: 1..mimc3_wide_max_radius(ocw); wide_class: 1..mimc3_wide_class_max_radius(ocw); wide_chip: 1..mimc3_wide_chip_max_radius(ocw)); levels outside 1..5
//   2. the context's state, MIMC3_ESTATE: no images; a chip-atlas context
//   3. the pair's class, MIMC3_EUNSUPPORTED (chip_class in mode 1: any pair that is not 8-bit; chip_planes in mode 1: any pair that is
//      neither 8-bit nor scaled-integer; wide_class beyond R 15 in mode 0: a pair that is not 8-bit at an (ocw, R) the float wide kernel does
//      not take; wide_planes beyond R 15: in mode 1 a radius beyond mimc3_wide_planes_max_radius(ocw), in mode 0 a scaled-integer pair
//      beyond that radius at an (ocw, R) the float wide kernel does not take -- every other class as wide_class; wide_chip: none, in
//      either mode)
//   4. MIMC3_EINVAL again: a coarsest pyramid level smaller than a chip; a mode other than 0 or 1; forward-backward rows without d_fb.
//      The _dev entries of the full searches have always made the last two with the arguments, under 1, and keep doing so: without
//      images they answer a bad mode with MIMC3_EINVAL where their host entries and the pyramids answer MIMC3_ESTATE.
// A host entry then makes the checks that need the points (search_check_host); the surfaces asked of an integer kernel are refused
// once the kernel is known (pick_kernel), unless the entry's rules let every kernel serve them (class_surf).
int search_check(mimc3_ctx *c, const SearchCall &call, const SearchRules &rules)
{
    const std::string en(call.entry);
    const bool early = !call.host && !rules.pyramid;
    const bool bad_mode = rules.has_mode && call.mode != 0 && call.mode != 1, no_fb = rules.fb && !call.d_fb;
    const bool mismatch = rules.cand == kCandOptional && (call.npeaks == 0) != (call.d_cand == nullptr);
    if (!c || !call.d_xyuvav || (!call.d_out && !rules.layer) || call.N <= 0 || (rules.cand == kCandMandatory && !call.d_cand) ||
        (rules.class_surf && !rules.layer && !call.d_surf) || (mismatch && !call.host) || (early && no_fb))
        return fail(MIMC3_EINVAL, en + ": bad argument");
    const int32_t least = rules.cand == kCandMandatory ? 1 : 0;
    if (rules.cand != kCandAbsent && (call.npeaks < least || call.npeaks > kFullMaxPeaks))
        return fail(MIMC3_EINVAL, en + ": npeaks must be in " + std::to_string(least) + "..8");
    if (mismatch) return fail(MIMC3_EINVAL, en + ": cand goes with npeaks > 0");
    if (early && bad_mode) return fail(MIMC3_EINVAL, en + ": mode must be 0 or 1");
    if (rules.any_ocw) {
        if (call.ocw < 1 || call.ocw > kFullChipMaxOcw) return fail(MIMC3_EINVAL, en + ": ocw must be in 1.." + std::to_string(kFullChipMaxOcw));
    } else if (!full_ocw_ok(call.ocw)) return fail(MIMC3_EINVAL, en + ": ocw must be one of 7, 15, 16, 30, 32, 40");
    if (!rules.layer && (call.R < 1 || call.R > (rules.wide_chip ? wide_chip_max_radius(call.ocw) : rules.wide_class ? wide_u8_max_radius(call.ocw) : rules.wide ? wide_max_radius(call.ocw) : 15)))
        return fail(MIMC3_EINVAL, en + (rules.wide_chip ? ": R must be in 1..mimc3_wide_chip_max_radius(ocw)"
                                        : rules.wide_class ? ": R must be in 1..mimc3_wide_class_max_radius(ocw)"
                                        : rules.wide     ? ": R must be in 1..mimc3_wide_max_radius(ocw)" : ": R must be in 1..15"));
    if (rules.pyramid && (call.levels < 1 || call.levels > 5)) return fail(MIMC3_EINVAL, en + ": levels must be in 1..5");
    if (!c->d_i0 || !c->d_i1) return fail(MIMC3_ESTATE, en + ": images not set");
    if (c->child) return fail(MIMC3_ESTATE, en + ": not on a chip-atlas context");
    RC_TRY(check_class(c, call.mode == 1 && rules.chip_planes ? kScaledInt : call.mode == 1 && rules.chip_class ? kU8 : rules.widest, en));
    // (wide_class beyond R 15, mode 0: a pair that is not 8-bit has the float wide kernel alone, which takes the six chip sizes up to its own radius)
    if (rules.wide_planes && call.R > 15 && (call.mode == 1 || (call.mode == 0 && !c->u8_ok && c->u16_ok))) {
        // (the matrix-core wide kernel on the u16 planes reaches wide_u16_max_radius(ocw); in mode 0 the float wide kernel serves what it takes)
        const int32_t lim = wide_u16_max_radius(call.ocw);
        if (call.R > lim && (call.mode == 1 || !wide_float_takes(call.ocw, call.R)))
            return fail(MIMC3_EUNSUPPORTED, en + ": beyond R 15 the u16-plane matrix-core kernel takes R <= mimc3_wide_planes_max_radius(ocw) = " +
                                            std::to_string(lim) + " at ocw " + std::to_string(call.ocw));
    } else if (rules.wide_class && call.R > 15 && call.mode == 0 && !c->u8_ok && !wide_float_takes(call.ocw, call.R))
        return fail(MIMC3_EUNSUPPORTED, en + ": beyond R 15 a pair that is not 8-bit needs ocw one of 7, 15, 16, 30, 32, 40 and R <= mimc3_wide_max_radius(ocw)");
    if (rules.pyramid && std::min(c->H >> (call.levels - 1), c->W >> (call.levels - 1)) < 2 * call.ocw + 1)
        return fail(MIMC3_EINVAL, en + ": level " + std::to_string(call.levels - 1) + " is smaller than a chip");
    if (bad_mode) return fail(MIMC3_EINVAL, en + ": mode must be 0 or 1");
    if (no_fb) return fail(MIMC3_EINVAL, en + ": bad argument");
    return 0;
}

int search_check_host(const mimc3_ctx *c, const char *entry, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                      int32_t ocw, int32_t R, bool pyramid)
{
    RC_TRY(check_chips(c, xyuvav, 0, N, ocw, entry));
    const int64_t pad = kU8Pad, h = R + ocw, lim = (int64_t)1 << 24;
    for (int32_t g = 0; g < N; ++g) {
        const int64_t du = (int64_t)offset[0] + (shift ? shift[2 * (size_t)g] : 0), dv = (int64_t)offset[1] + (shift ? shift[2 * (size_t)g + 1] : 0);
        if (pyramid) {      // (a point whose derived search box leaves the zero border gets the all-NaN record)
            if (offset[0] < -lim || offset[0] > lim || offset[1] < -lim || offset[1] > lim || du < -lim || du > lim || dv < -lim || dv > lim)
                return fail(MIMC3_EINVAL, std::string(entry) + ": grid point " + std::to_string(g) + " starting displacement beyond +-2^24");
            continue;
        }
        const int64_t cu = (int64_t)(int32_t)xyuvav[6 * (size_t)g + 2] + du, cv = (int64_t)(int32_t)xyuvav[6 * (size_t)g + 3] + dv;
        if (cu - h < -pad || cu + h >= c->W + pad || cv - h < -pad || cv + h >= c->H + pad)
            return fail(MIMC3_EBOUNDS, std::string(entry) + ": grid point " + std::to_string(g) + " search box leaves the zero border");
    }
    return 0;
}

// The kernel of a checked call: beyond R 15 the wide float kernel (only the wide entries let such a radius through); in mode 1 the
// float kernel; else the kernel of the pair's class -- matrix cores on an 8-bit pair, u16 planes on a scaled-integer one, f32 planes
// with tables on an integral-f32 one, the float kernel on any other.  Only the float kernels serve the surfaces, unless the rules
// say class_surf: then the integer kernels run their surface-storing forms.  Under any_ocw the run-time-ocw float kernel takes mode 1 and
// every chip size the others are not built for; mode 0 at one of the six takes the class dispatch as before.  Under chip_class an 8-bit
// pair takes the run-time-ocw matrix-core kernel instead, in mode 1 (search_check has refused every other class) and at the chip sizes
// outside the six that chip_mode0 names.
// The mode-0 rule follows the series of tools/full_chip_u8_time.py (profiles/full_search_chip_u8/): an ocw goes to the matrix-core kernel
// where every pass of its series was faster than every pass of the float kernel's -- on BASELINE C2 every ocw measured, 7 .. 80, the
// 97-99.6 % dirty sizes 60 and 80 included.
// Under chip_planes (mimc3_match_ncc_full_chip_planes) a scaled-integer pair takes the run-time-ocw matrix-core kernel on the u16 planes as
// well: in mode 1 at every ocw (an 8-bit pair included: q < 256 on its u16 planes; search_check has refused every wider class) and in
// mode 0 at the chip sizes outside the six that chip_mode0 names; an 8-bit pair in mode 0 keeps the u8 kernel.
// The same rule on the series of tools/full_chip_u16_time.py (profiles/full_search_chip_u16/): on BASELINE C2 as 12-bit DN and as its d/dx
// pair every pass of the matrix-core kernel was faster than every pass of the float kernel at every ocw measured, 7 .. 80 (3.55 ms against
// 16.9 at ocw 7, 350 ms against 2414 at ocw 80, where 99.6 % of the points run the masked form): no range stays on the float kernel.
// One predicate for both kernels (ChipU8, ChipU16): the measured ranges happen to be the same, every ocw in range; a range that a later
// series hands back to the float kernel is cut out here, per kernel.
static bool chip_mode0(SearchKernel, int32_t ocw) { return ocw >= 1 && ocw <= kFullChipMaxOcw; }
// The same rule beyond R 15 (mimc3_match_ncc_wide_class, mode 0, an 8-bit pair) on the series of tools/wide_u8_time.py
// (profiles/full_search_wide_u8/): an (ocw, R) the float wide kernel takes goes to the matrix-core wide kernel where every pass of its
// series was faster than every pass of the float kernel's in the same session -- on BASELINE C2
// every configuration measured (ocw 7, 16, 40; R 16 .. 47; npeaks 0 and 4: 3.4 to 32.2 times faster; ocw 15, 30, 32 at R 16 and 47 in a second run: 9.4 to 25.8), so no (ocw, R) stays on the float kernel
static bool wide_mode0(int32_t ocw, int32_t R) { return ocw >= 1 && ocw <= kFullChipMaxOcw && R >= 16 && R <= wide_u8_max_radius(ocw); }
// The same rule for a scaled-integer pair (mimc3_match_ncc_wide_planes, mode 0) on the series of tools/wide_u16_time.py
// (profiles/full_search_wide_u16/): an (ocw, R) the float wide kernel also takes goes to the matrix-core wide kernel on
// the u16 planes where every pass of its series was faster than every pass of the float kernel's in the same session -- on BASELINE C2 as 12-bit DN and as
// its d/dx pair every configuration measured (ocw 7, 16, 40; R 16 .. 47; npeaks 0 and 4: 2.4 to 19.1 times faster; ocw 15, 30, 32 at R 16 and 47 in a second run:
// 5.0 to 16.9), so no (ocw, R) stays on the float kernel
static bool wide_planes_mode0(int32_t ocw, int32_t R) { return ocw >= 1 && ocw <= kFullChipMaxOcw && R >= 16 && R <= wide_u16_max_radius(ocw); }

// The coarse-to-fine search at any chip size (mimc3_match_ncc_pyramid_chip) runs ONE kernel on every level of a call, level 0 included,
// on the levels of the pair's class:
//   8-bit            mode 0 at one of the six: Mx (the entry is then mimc3_match_ncc_pyramid_dn); any other ocw, and all of mode 1: ChipU8
//   scaled-integer   ChipU16 in both modes -- in mode 0 at one of the six only where pyramid_chip_u16_at_six says so, else U16
//   integral f32     mode 0 at one of the six: F32i (mimc3_match_ncc_pyramid_dn); else Chip, on the integral-f32 levels' planes
//   any other        mode 0 at one of the six: F32g on the float levels (mimc3_match_ncc_pyramid_any(mode 0)); else Chip on the float levels
// (ChipU16 never runs on an 8-bit pair here: the context keeps one integer level set per pair, the u8 one.)
// The mode-0 choice for a scaled-integer pair at the six: ChipU16 where every pass of its series was faster than every pass of
// mimc3_match_ncc_pyramid_dn's in the same session, configuration by configuration (tools/pyramid_chip_time.py,
// profiles/full_search_pyramid_chip/time_C2.jsonl).  On BASELINE C2 as 12-bit DN (R 15, L 2 and 3, npeaks 0 and 4) that holds at all six:
// L = 3 costs 13.2 against 20.6 ms at ocw 7, 25.9 against 104.4 at ocw 16, 178.4 against 607.3 at ocw 40 (1.5 to 4.0 times faster over
// the series).  An ocw that a later series hands back to the templated kernel is cut out here.
static bool pyramid_chip_u16_at_six(int32_t ocw) { return full_ocw_ok(ocw); }

bool pyramid_chip_kernel(PairClass cls, int32_t ocw, int32_t mode, SearchKernel &kernel)
{
    if (ocw < 1 || ocw > kFullChipMaxOcw || (mode != 0 && mode != 1)) return false;
    // the kernel of mimc3_match_ncc_pyramid_dn / _any(mode 0) per pair class, and the run-time-ocw kernel that takes its place
    static const SearchKernel built[4] = {Mx, U16, F32i, F32g}, chip[4] = {ChipU8, ChipU16, Chip, Chip};     // (in PairClass's order)
    const bool six = mode == 0 && full_ocw_ok(ocw) && !(cls == kScaledInt && pyramid_chip_u16_at_six(ocw));
    kernel = six ? built[cls] : chip[cls];
    return true;
}

// The kernel of mimc3_match_ncc_wide_chip (the table in include/mimc3_hip.h).  R <= 15: mode 1 the run-time-ocw float kernel
// (mimc3_match_ncc_full_chip), mode 0 what mimc3_match_ncc_full_chip_planes(mode 0) runs.  R >= 16: mode 1 the run-time-ocw wide float
// kernel; mode 0 the sibling that takes the call -- an 8-bit pair where mimc3_match_ncc_wide_class(mode 0) sends it, a scaled-integer pair
// within wide_u16_max_radius(ocw) where mimc3_match_ncc_wide_planes(mode 0) sends it, any other pair the templated wide float kernel at
// the (ocw, R) it takes -- and the run-time-ocw wide float kernel everywhere else.  At the six chip sizes mode 0 keeps the templated
// kernel: tools/wide_chip_time.py measures the two side by side, and nothing is moved before a series says so.
bool wide_chip_kernel(PairClass cls, int32_t ocw, int32_t R, int32_t mode, SearchKernel &kernel)
{
    if (ocw < 1 || ocw > kFullChipMaxOcw || R < 1 || R > wide_chip_max_radius(ocw) || (mode != 0 && mode != 1)) return false;
    if (R <= 15) {
        static const SearchKernel built[4] = {Mx, U16, F32i, F32g};         // (in PairClass's order)
        if (mode == 1) kernel = Chip;
        else if (full_ocw_ok(ocw)) kernel = built[cls];
        else kernel = cls == kU8 && chip_mode0(ChipU8, ocw) ? ChipU8 : cls == kScaledInt && chip_mode0(ChipU16, ocw) ? ChipU16 : Chip;
        return true;
    }
    const bool takes = wide_float_takes(ocw, R);
    if (mode == 1) kernel = WideChip;
    else if (cls == kU8) kernel = wide_mode0(ocw, R) || !takes ? WideU8 : Wide;
    else if (cls == kScaledInt && R <= wide_u16_max_radius(ocw)) kernel = wide_planes_mode0(ocw, R) || !takes ? WideU16 : Wide;
    else kernel = takes && cls != kScaledInt ? Wide : WideChip;
    return true;
}

int pick_kernel(mimc3_ctx *c, const SearchCall &call, const SearchRules &rules, SearchKernel &kernel)
{
    if (rules.wide_chip) {              // (search_check has refused every ocw, R and mode outside the table)
        PairClass cls = kFloat;
        if (call.mode != 1) RC_TRY(pair_class(c, cls));
        if (!wide_chip_kernel(cls, call.ocw, call.R, call.mode, kernel)) return fail(MIMC3_EINVAL, std::string(call.entry) + ": bad argument");
        return 0;                       // (whichever kernel runs serves the surfaces)
    }
    if (rules.pyramid_chip) {           // (search_check has refused every ocw and mode outside the table)
        PairClass cls;
        RC_TRY(pair_class(c, cls));
        if (!pyramid_chip_kernel(cls, call.ocw, call.mode, kernel)) return fail(MIMC3_EINVAL, std::string(call.entry) + ": bad argument");
    }
    else if (call.R > 15 && rules.wide_planes && (call.mode == 1 || (!c->u8_ok && c->u16_ok))) {
        // (mode 1: search_check has refused every pair that is neither 8-bit nor scaled-integer, and every radius beyond the kernel's;
        //  mode 0, a scaled-integer pair: search_check has refused what neither kernel takes)
        const bool u16 = call.mode == 1 || (call.R <= wide_u16_max_radius(call.ocw) &&
                                            (wide_planes_mode0(call.ocw, call.R) || !wide_float_takes(call.ocw, call.R)));
        kernel = u16 ? WideU16 : Wide;
    }
    else if (call.R > 15 && rules.wide_class) {
        // (mode 1: search_check has refused every pair that is not 8-bit; mode 0: every pair the float wide kernel cannot take)
        const bool u8 = call.mode == 1 || (c->u8_ok && (wide_mode0(call.ocw, call.R) || !wide_float_takes(call.ocw, call.R)));
        kernel = u8 ? WideU8 : Wide;
    }
    else if (call.R > 15) kernel = Wide;
    else if (rules.chip_class && (call.mode == 1 || !full_ocw_ok(call.ocw))) {
        // (mode 1: the entry's own matrix-core kernel on whatever search_check let through; mode 0: the kernel of the pair's class)
        PairClass cls = rules.chip_planes ? kScaledInt : kU8;
        if (call.mode != 1) RC_TRY(pair_class(c, cls));
        const bool u16 = rules.chip_planes && (call.mode == 1 || cls == kScaledInt);
        kernel = u16 ? (call.mode == 1 || chip_mode0(ChipU16, call.ocw) ? ChipU16 : Chip)
                     : cls == kU8 && (call.mode == 1 || chip_mode0(ChipU8, call.ocw)) ? ChipU8 : Chip;
    }
    else if (rules.any_ocw && (call.mode == 1 || !full_ocw_ok(call.ocw))) kernel = Chip;
    else if (call.mode == 1) kernel = F32g;
    else {
        PairClass cls;
        RC_TRY(pair_class(c, cls));
        kernel = cls == kU8 ? Mx : cls == kScaledInt ? U16 : cls == kIntegralF32 ? F32i : F32g;
    }
    if (kernel < F32g && call.d_surf && !rules.class_surf && !rules.chip_class)
        return fail(MIMC3_EINVAL, std::string(call.entry) + ": only the float kernel serves the surfaces (mode 1, or a pair of no integer class)");
    return 0;
}

// ---- pyramid levels ----
// The level set a kernel reads by default: its own plane type's.  (The run-time-ocw float kernel also reads the integral-f32 set, planes
// alone -- mimc3_match_ncc_pyramid_chip says so through plane_set's LevelClass argument.)
LevelClass level_class(SearchKernel kernel)
{
    static const LevelClass of[kSearchKernels] = {kLevelU8, kLevelU16, kLevelF32i, kLevelFloat, kLevelFloat, kLevelFloat,
                                                  kLevelU8, kLevelU16, kLevelU8, kLevelU16, kLevelFloat};     // (in SearchKernel's order)
    return of[kernel];
}
// the level set of a pair's class (in PairClass's order)
static const LevelClass kLevelOfPair[4] = {kLevelU8, kLevelU16, kLevelF32i, kLevelFloat};

// the tables of one level plane (image k) of an integer class; the float levels have none
static int tables_u8(mimc3_ctx *c, PyrLevel &d, int k)
{
    const int Hp = d.H + 2 * kU8Pad;
    DevBuf &pl = k ? d.pl1 : d.pl0, &sat = k ? d.sat1 : d.sat0;
    HIP_TRY(sat.reserve(sat_bytes(Hp, d.Wp)));
    HIP_TRY(c->sat_tmp.reserve(sat_scratch_bytes(Hp, d.Wp)));
    HIP_TRY(launch_sat_u8(static_cast<const unsigned char *>(pl.p), d.Wp, SatRegion{0, 0, d.Wp, Hp}, static_cast<unsigned long long *>(sat.p),
                          c->sat_tmp.p, c->stream));
    return 0;
}
static int tables_u16(mimc3_ctx *c, PyrLevel &d, int k)
{
    const int Hp = d.H + 2 * kU8Pad;
    DevBuf &pl = k ? d.pl1 : d.pl0, &sat = k ? d.sat1 : d.sat0, &sz = k ? d.sz1 : d.sz0;
    HIP_TRY(sat.reserve(sat_bytes(Hp, d.Wp)));
    HIP_TRY(c->sat_tmp.reserve(sat_scratch_bytes(Hp, d.Wp)));
    HIP_TRY(sz.reserve(sat_null_bytes(Hp, d.Wp)));
    HIP_TRY(launch_sat_u16(static_cast<const unsigned short *>(pl.p), d.Wp, SatRegion{0, 0, d.Wp, Hp}, static_cast<unsigned long long *>(sat.p),
                           static_cast<unsigned int *>(sz.p), c->sat_tmp.p, c->stream));
    return 0;
}
static int tables_f32i(mimc3_ctx *c, PyrLevel &d, int k)
{
    const int Hp = d.H + 2 * kU8Pad;
    DevBuf &pl = k ? d.pl1 : d.pl0, &sat = k ? d.sat1 : d.sat0;
    HIP_TRY(sat.reserve(sat2_bytes(Hp, d.Wp)));
    HIP_TRY(c->sat_tmp.reserve(sat2_scratch_bytes(Hp, d.Wp)));
    HIP_TRY(launch_sat_f32i(static_cast<const float *>(pl.p), d.Wp, SatRegion{0, 0, d.Wp, Hp}, k ? c->fshift1 : c->fshift0,
                            static_cast<Sat2 *>(sat.p), c->sat_tmp.p, c->stream));
    return 0;
}

// what tells the level sets apart: the element, the 2 x 2 null-aware reduction of a plane to the next level, the tables of a level plane
// (null: none), the kernel whose level-0 planes the set starts from, and where the context keeps the set
struct LevelType {
    size_t elem;
    hipError_t (*reduce)(const void *src, int Hs, int Ws, int Wps, void *dst, int Hd, int Wd, int Wpd, int shift, hipStream_t s);
    int (*tables)(mimc3_ctx *c, PyrLevel &d, int k);
    SearchKernel top;
    PyrLevel (mimc3_ctx::*levels)[4];
    int mimc3_ctx::*built;
};
static const LevelType kLevelType[4] = {      // (in LevelClass's order)
    {1, [](const void *s, int Hs, int Ws, int Wps, void *d, int Hd, int Wd, int Wpd, int, hipStream_t st) {
         return launch_pyr_reduce(static_cast<const unsigned char *>(s), Hs, Ws, Wps, static_cast<unsigned char *>(d), Hd, Wd, Wpd, kU8Pad, st); },
     tables_u8, Mx, &mimc3_ctx::pyr, &mimc3_ctx::pyr_levels},
    {2, [](const void *s, int Hs, int Ws, int Wps, void *d, int Hd, int Wd, int Wpd, int, hipStream_t st) {
         return launch_pyr_reduce_u16(static_cast<const unsigned short *>(s), Hs, Ws, Wps, static_cast<unsigned short *>(d), Hd, Wd, Wpd, kU8Pad, st); },
     tables_u16, U16, &mimc3_ctx::pyr, &mimc3_ctx::pyr_levels},
    {4, [](const void *s, int Hs, int Ws, int Wps, void *d, int Hd, int Wd, int Wpd, int shift, hipStream_t st) {
         return launch_pyr_reduce_f32(static_cast<const float *>(s), Hs, Ws, Wps, static_cast<float *>(d), Hd, Wd, Wpd, kU8Pad, shift, st); },
     tables_f32i, F32i, &mimc3_ctx::pyr, &mimc3_ctx::pyr_levels},
    {4, [](const void *s, int Hs, int Ws, int Wps, void *d, int Hd, int Wd, int Wpd, int, hipStream_t st) {
         return launch_pyr_reduce_f32g(static_cast<const float *>(s), Hs, Ws, Wps, static_cast<float *>(d), Hd, Wd, Wpd, kU8Pad, st); },
     nullptr, F32g, &mimc3_ctx::pyrg, &mimc3_ctx::pyrg_levels},
};

// Levels 1 .. L - 1 of the current pair in the set `lc` -- the levels of an integer class (u8 planes; u16 planes q = pixel * 2^shift, which
// keep the image's shift; f32 planes reduced on the integers w = pixel * 2^fshift), each with its tables, or the float levels (the f64
// mean of the block's included pixels; no tables) -- each from the level above, starting at the level-0 set.  A set is the same whichever
// kernel asks for it first: an integer class's levels always carry their tables.  Like every plane-set
// builder: enqueued on the context's stream and drained before the levels count as built.
static int build_levels(mimc3_ctx *c, LevelClass lc, int L)
{
    const LevelType &t = kLevelType[lc];
    PyrLevel *lv = c->*t.levels;
    int &built = c->*t.built;
    PlaneSet top;
    RC_TRY(plane_set(c, t.top, 0, top));
    if (built >= L - 1) return 0;
    for (int l = built + 1; l < L; ++l) {
        PyrLevel &d = lv[l - 1];
        const PyrLevel *up = l == 1 ? nullptr : &lv[l - 2];
        const int Hs = up ? up->H : top.H, Ws = up ? up->W : top.W, Wps = up ? up->Wp : top.Wp;
        d.H = Hs >> 1; d.W = Ws >> 1; d.Wp = (d.W + 2 * kU8Pad + 3) & ~3;
        const size_t bytes = t.elem * (size_t)(d.H + 2 * kU8Pad) * d.Wp;
        for (int k = 0; k < 2; k++) {
            DevBuf &pl = k ? d.pl1 : d.pl0;
            const void *src = up ? (k ? up->pl1.p : up->pl0.p) : (k ? top.p1 : top.p0);
            HIP_TRY(pl.reserve(bytes));
            HIP_TRY(hipMemsetAsync(pl.p, 0, bytes, c->stream));
            HIP_TRY(t.reduce(src, Hs, Ws, Wps, pl.p, d.H, d.W, d.Wp, k ? c->fshift1 : c->fshift0, c->stream));
            if (t.tables) RC_TRY(t.tables(c, d, k));
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    built = L - 1;
    return 0;
}

// The planes and tables `kernel` reads on `level`: 0 = the resident pair's set, whose missing parts are built on first use; l >= 1 =
// the pyramid level of the set `lc`, built with the levels above it on first use.
int plane_set(mimc3_ctx *c, SearchKernel kernel, int level, PlaneSet &pl) { return plane_set(c, kernel, level_class(kernel), level, pl); }

int plane_set(mimc3_ctx *c, SearchKernel kernel, LevelClass lc, int level, PlaneSet &pl)
{
    pl = PlaneSet{};
    if (kernel == F32i) { pl.scale0 = 1.0 / (double)(1 << c->fshift0); pl.scale1 = 1.0 / (double)(1 << c->fshift1); }
    if (level > 0) {
        RC_TRY(build_levels(c, lc, level + 1));
        const PyrLevel &d = (c->*kLevelType[lc].levels)[level - 1];
        pl.p0 = d.pl0.p; pl.p1 = d.pl1.p; pl.sat0 = d.sat0.p; pl.sat1 = d.sat1.p; pl.satz0 = d.sz0.p; pl.satz1 = d.sz1.p;
        pl.H = d.H; pl.W = d.W; pl.Wp = d.Wp;
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    pl.H = c->H; pl.W = c->W; pl.Wp = c->Wp;
    if (kernel == Mx || kernel == ChipU8 || kernel == WideU8) {
        if (!c->sat_u8_ok) RC_TRY(build_u8_tables(c));
        pl.p0 = c->pl0.p; pl.p1 = c->pl1.p; pl.sat0 = c->sat0.p; pl.sat1 = c->sat1.p;
    } else if (kernel == U16 || kernel == ChipU16 || kernel == WideU16) {
        if (!c->hpl_valid || !c->sat_u16_ok) RC_TRY(build_u16(c, true));
        pl.p0 = c->hpl0.p; pl.p1 = c->hpl1.p; pl.sat0 = c->hsat0.p; pl.sat1 = c->hsat1.p; pl.satz0 = c->hsz0.p; pl.satz1 = c->hsz1.p;
    } else {
        // (the float kernels on an 8-bit or scaled-integer pair: build_f32 also classifies the pair as integral f32 and builds the
        //  16-byte tables, which they never read -- once per pair, on the path of tests and surfaces; the planes are the same ones)
        if (!c->fplanes_ok) RC_TRY(build_f32(c));
        pl.p0 = c->fpl0.p; pl.p1 = c->fpl1.p;
        if (kernel == F32i) { pl.sat0 = c->fsat0.p; pl.sat1 = c->fsat1.p; }
    }
    return 0;
}

// the kernels that run as a clean launch plus a masked launch in flag mode: one class byte per point (in SearchKernel's order)
static const bool kKernelFlags[kSearchKernels] = {true, false, false, false, false, false, true, true, true, true, false};

// One search launch: `kernel` over the call's points on `planes`, with the timing events around it (unless suspended) and last_path.
int launch_search(mimc3_ctx *c, SearchKernel kernel, const PlaneSet &pl, const SearchCall &call)
{
    static const char *const what[] = {"full-search kernel launch", "full-search u16 kernel launch", "full-search f32 kernel launch",
                                       "full-search general f32 kernel launch", "wide-search kernel launch", "full-search any-chip kernel launch",
                                       "full-search any-chip u8 kernel launch", "full-search any-chip u16 kernel launch", "wide-search u8 kernel launch",
                                       "wide-search u16 kernel launch", "wide-search any-chip kernel launch"};
    hipStream_t s = call.stream;
    MatchU8Args u = u8_args(c, call.d_xyuvav, call.xy_stride, call.xy_col, call.N, call.off_u, call.off_v, call.ocw, call.swap, call.d_out);
    u.H = pl.H; u.W = pl.W; u.Wp = pl.Wp;
    u.full_shift = call.d_shift; u.full_R = call.R; u.full_peak = call.d_peak;
    if (call.d_cand) { u.full_cand = call.d_cand; u.full_npeaks = call.npeaks; }
    if (kernel < F32g || kernel == ChipU8 || kernel == ChipU16 || kernel == WideU8 || kernel == WideU16) u.full_surf = call.d_surf;       // (the float kernels take it as an argument of its own)
    u.p0 = static_cast<const unsigned char *>(pl.p0); u.p1 = static_cast<const unsigned char *>(pl.p1);
    if (pl.sat0) { u.sat0 = pl.sat0; u.sat1 = pl.sat1; u.satz0 = pl.satz0; u.satz1 = pl.satz1; u.sat_ws = sat_pitch(pl.Wp); }
    u.scale0 = pl.scale0; u.scale1 = pl.scale1;
    const bool flags = kKernelFlags[kernel];
    // a fused stack layer: the accumulating forms of the four run-time-ocw matrix-core kernels (no other kernel has them)
    const int acc = call.stk_sum ? kFormsAcc : 0;
    if (acc) {
        if (kernel != ChipU8 && kernel != ChipU16 && kernel != WideU8 && kernel != WideU16)
            return fail(MIMC3_EUNSUPPORTED, std::string(call.entry) + ": this kernel has no accumulating form");
        u.stk_sum = call.stk_sum; u.stk_cnt = call.stk_cnt; u.stk_lay = call.stk_lay; u.stk_wsum = call.stk_wsum;
        // (a scaled layer: in the slots of the plane scales and the range tiles, which these kernels do not read)
        if (call.stk_shift) { u.stk_shift = call.stk_shift; u.stk_R = call.stk_R; u.stk_scale = call.stk_scale; u.stk_weight = call.stk_weight; }
    }
    if (flags) HIP_TRY(c->mxl[0].reserve((size_t)call.N));             // one class byte per point, zero before the launch
    if (c->timing) HIP_TRY(hipEventRecord(c->ev0, s));
    hipError_t e;
    if (flags) {
        HIP_TRY(hipMemsetAsync(c->mxl[0].p, 0, (size_t)call.N, s));
        u.mx_flags = static_cast<uint8_t *>(c->mxl[0].p);
    }
    if (kernel == Mx) e = launch_match_full_mx(u, s);
    else if (kernel == ChipU8) {
        // tuning / timing: MIMC3_CHIP_U8_FORMS = 1 runs the clean form alone (the flagged points get no result), 2 the masked form alone
        // (over no point: nothing has flagged one); read at every call, so that one process can time the forms apart
        const char *fe = getenv("MIMC3_CHIP_U8_FORMS");
        const int forms = fe ? atoi(fe) & 3 : 3;
        e = launch_match_full_chip_u8(u, (forms ? forms : 3) | acc, s);
    } else if (kernel == ChipU16) {
        // (MIMC3_CHIP_U16_FORMS: the same measurement-only switch for this kernel's two forms -- tools/full_chip_u16_time.py times the clean
        //  form with it; DESIGN 4.1r names it.  With 1 the flagged points get no result: never set it around a real search)
        const char *fe = getenv("MIMC3_CHIP_U16_FORMS");
        const int forms = fe ? atoi(fe) & 3 : 3;
        e = launch_match_full_chip_u16(u, (forms ? forms : 3) | acc, s);
    } else if (kernel == WideU8) {
        // (MIMC3_WIDE_U8_FORMS: the same measurement-only switch for this kernel's two forms -- tools/wide_u8_time.py times the clean form
        //  with it; DESIGN 4.1s names it.  With 1 the flagged points get no result: never set it around a real search)
        const char *fe = getenv("MIMC3_WIDE_U8_FORMS");
        const int forms = fe ? atoi(fe) & 3 : 3;
        e = launch_match_wide_u8(u, (forms ? forms : 3) | acc, s);
    } else if (kernel == WideU16) {
        // (MIMC3_WIDE_U16_FORMS: the same measurement-only switch for this kernel's two forms -- tools/wide_u16_time.py times the clean form
        //  with it; DESIGN 4.1t names it.  With 1 the flagged points get no result: never set it around a real search)
        const char *fe = getenv("MIMC3_WIDE_U16_FORMS");
        const int forms = fe ? atoi(fe) & 3 : 3;
        e = launch_match_wide_u16(u, (forms ? forms : 3) | acc, s);
    } else if (kernel == U16) e = launch_match_full_u16(u, s);
    else if (kernel == F32i) e = launch_match_full_f32(u, s);
    else if (kernel == F32g) e = launch_match_full_f32g(u, call.d_surf, s);
    else if (kernel == Chip) e = launch_match_full_chip(u, call.d_surf, s);
    else if (kernel == WideChip) e = launch_match_wide_chip(u, call.d_surf, s);
    else e = launch_match_wide(u, call.d_surf, s);
    if (e != hipSuccess) return hip_fail(e, what[kernel]);
    c->last_path = 6 + (int)kernel;
    if (c->timing) { HIP_TRY(hipEventRecord(c->ev1, s)); c->timed = true; }
    return 0;
}

// ---- what each public entry accepts ----                widest        mode   wide   candidates      fb     pyramid  layer  class_surf  any_ocw
static const SearchRules kFull = {kU8, false, false, kCandAbsent};
static const SearchRules kFullMulti = {kU8, false, false, kCandMandatory};
static const SearchRules kFullPlanes = {kScaledInt, false, false, kCandOptional};
static const SearchRules kFullDn = {kIntegralF32, false, false, kCandOptional};
static const SearchRules kFullAny = {kFloat, true, false, kCandOptional};
static const SearchRules kFullChip = {kFloat, true, false, kCandOptional, false, false, false, false, true};    // (any_ocw)
static const SearchRules kFullChipClass = {kFloat, true, false, kCandOptional, false, false, false, false, true, true};     // (any_ocw, chip_class)
static const SearchRules kFullChipPlanes = {kFloat, true, false, kCandOptional, false, false, false, false, true, true, true};    // (..., chip_planes)
static const SearchRules kWideClass = {kFloat, true, false, kCandOptional, false, false, false, false, true, true, false, true};    // (any_ocw, chip_class, wide_class)
static const SearchRules kWidePlanes = {kFloat, true, false, kCandOptional, false, false, false, false, true, true, true, true, true};    // (..., chip_planes, wide_class, wide_planes)
static const SearchRules kFullSurf = {kFloat, false, false, kCandOptional, false, false, false, true};     // (class_surf: surf is mandatory)
static const SearchRules kWide = {kFloat, false, true, kCandOptional};
static const SearchRules kFullFb = {kFloat, true, false, kCandOptional, true};
static const SearchRules kWideFb = {kFloat, false, true, kCandOptional, true};
static const SearchRules kPyramid = {kU8, false, false, kCandAbsent, false, true};
static const SearchRules kPyramidDn = {kIntegralF32, false, false, kCandOptional, false, true};
static const SearchRules kPyramidAny = {kFloat, true, false, kCandOptional, false, true};
static const SearchRules kPyramidChip = {kFloat, true, false, kCandOptional, false, true, false, false, true, false, false, false, false, true};   // (pyramid, any_ocw, pyramid_chip)
static const SearchRules kWideChip = {kFloat, true, false, kCandOptional, false, false, false, false, true, false, false, false, false, false, true};   // (any_ocw, wide_chip)

// the description of a _dev entry's call (`levels`, d_fb: the entries that have them set them)
static SearchCall dev_call(const char *entry, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v, const int32_t *d_shift,
                           int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode, float *d_out, float *d_cand, float *d_surf,
                           void *stream)
{
    return SearchCall{entry, false, d_xyuvav, 6, 2, N, off_u, off_v, d_shift, ocw, R, npeaks, swap ? 1 : 0, mode, 0, d_out, d_cand, d_surf,
                      nullptr, nullptr, static_cast<hipStream_t>(stream)};
}

// the device entry of one search: the record, the candidates and the surfaces the call asks for
static int search_dev(mimc3_ctx *c, const SearchCall &call, const SearchRules &rules)
{
    RC_TRY(search_check(c, call, rules));
    HIP_TRY(hipSetDevice(c->device));
    SearchKernel kernel;
    PlaneSet planes;
    RC_TRY(pick_kernel(c, call, rules, kernel));
    RC_TRY(plane_set(c, kernel, 0, planes));
    return launch_search(c, kernel, planes, call);
}

// Forward-backward consistency (mimc3_match_ncc_full_fb, fb_kernel.hip): the forward search of the call (swap 0, no surfaces), then ONE
// backward search (swap 1) over the record and the candidates of every point -- (1 + npeaks) N rows, seeded on the device from the
// forward results -- and the fb rows composed from it; all on the caller's stream, no host round trip.  Both passes run the same
// kernel; wide (mimc3_match_ncc_wide_fb): mode 1 with R up to mimc3_wide_max_radius(ocw), so R <= 15 is mimc3_match_ncc_full_fb(mode 1)
static int full_fb_dev(mimc3_ctx *c, const SearchCall &call, const SearchRules &rules)
{
    RC_TRY(search_check(c, call, rules));
    const int32_t N = call.N, npeaks = call.npeaks;
    const size_t rows = (size_t)(1 + npeaks) * (size_t)N;
    if (rows > (size_t)INT32_MAX) return fail(MIMC3_EINVAL, std::string(call.entry) + ": (1 + npeaks) N must fit an int32");
    hipStream_t s = call.stream;
    // all scratch before anything is enqueued (a buffer that grows is freed first, and hipFree waits for the device): the backward rows,
    // and the class bytes of the matrix-core search at the backward pass's size, which the forward pass would otherwise size for N
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->fb_xy.reserve(sizeof(double) * 6 * rows));
    HIP_TRY(c->fb_sh.reserve(sizeof(int32_t) * 2 * rows));
    HIP_TRY(c->fb_rec.reserve(sizeof(float) * 8 * rows));
    HIP_TRY(c->fb_why.reserve(rows));
    if (c->u8_ok && call.mode == 0) HIP_TRY(c->mxl[0].reserve(rows));
    if (c->timing) HIP_TRY(hipEventRecord(c->ev0, s));
    TimingSuspended whole(c);           // (the events bracket the whole call, not its last search)
    SearchKernel kernel;
    PlaneSet planes;
    RC_TRY(pick_kernel(c, call, rules, kernel));
    RC_TRY(plane_set(c, kernel, 0, planes));
    RC_TRY(launch_search(c, kernel, planes, call));
    double *xy2 = static_cast<double *>(c->fb_xy.p);
    int32_t *sh2 = static_cast<int32_t *>(c->fb_sh.p);
    float *back = static_cast<float *>(c->fb_rec.p);
    uint8_t *why = static_cast<uint8_t *>(c->fb_why.p);
    hipError_t e = launch_fb_seed(call.d_xyuvav, N, call.off_u, call.off_v, call.d_out, call.d_cand, npeaks, call.ocw, c->H, c->W, xy2, sh2, why, s);
    if (e != hipSuccess) return hip_fail(e, "fb seed kernel launch");
    // the backward pass: the chip from i1 at m, the search in i0 around m - offset - r = uv0 (inside the 256-px zero border: the box is
    // centred on uv0, which lies in the image, and R + ocw <= 15 + 40; wide: R + ocw <= 47 + 32 = 79).  last_path stays the forward pass's:
    // the same kernel
    SearchCall bw = call;
    bw.d_xyuvav = xy2; bw.N = (int32_t)rows; bw.off_u = -call.off_u; bw.off_v = -call.off_v; bw.d_shift = sh2; bw.npeaks = 0; bw.swap = 1;
    bw.d_out = back; bw.d_cand = nullptr;
    RC_TRY(launch_search(c, kernel, planes, bw));
    e = launch_fb_compose(call.d_out, call.d_cand, N, npeaks, back, why, call.d_fb, s);
    if (e != hipSuccess) return hip_fail(e, "fb compose kernel launch");
    if (whole.was) { HIP_TRY(hipEventRecord(c->ev1, s)); c->timed = true; }
    return 0;
}

// Coarse-to-fine search over an image pyramid (pyramid_kernel.hip): the levels of the call's kernel, then per level the step and the
// exhaustive search with the arg-max cells, chained on one stream; level 0 is the plain search at shift = sh (record and candidates).
// The kernel is the one the same call without levels would run: the float kernel searches the float levels, an integer class its own.
// mimc3_match_ncc_pyramid_chip (rules.pyramid_chip): the kernel of pyramid_chip_kernel on the levels of the PAIR's class, whichever kernel
// that is -- the run-time-ocw float kernel reads the integral-f32 levels' planes on an integral-f32 pair.
static int pyramid_dev(mimc3_ctx *c, const SearchCall &call, const SearchRules &rules, int32_t *d_shift_out)
{
    RC_TRY(search_check(c, call, rules));
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = call.stream;
    const int32_t N = call.N, levels = call.levels;
    SearchKernel kernel;
    PlaneSet planes;
    RC_TRY(pick_kernel(c, call, rules, kernel));
    LevelClass lc = level_class(kernel);
    if (rules.pyramid_chip) {
        PairClass cls;
        RC_TRY(pair_class(c, cls));
        lc = kLevelOfPair[cls];
    }
    RC_TRY(plane_set(c, kernel, lc, levels - 1, planes));   // (every level the call reads exists before its first launch)
    // all scratch before anything is enqueued (a buffer that grows is freed first, and hipFree waits for the device): the class bytes of
    // the kernels that hand points from their clean form to their masked one (launch_search then finds them large enough), then the
    // points' positions, arg-max cells and shifts
    if (kKernelFlags[kernel]) HIP_TRY(c->mxl[0].reserve((size_t)N));
    HIP_TRY(c->pyr_pos.reserve(sizeof(double) * 2 * (size_t)N));
    HIP_TRY(c->pyr_peak.reserve(sizeof(int32_t) * (size_t)N));
    if (!d_shift_out) HIP_TRY(c->pyr_sh.reserve(sizeof(int32_t) * 2 * (size_t)N));
    int32_t *sh = d_shift_out ? d_shift_out : static_cast<int32_t *>(c->pyr_sh.p);
    double *pos = static_cast<double *>(c->pyr_pos.p);
    int32_t *peak = static_cast<int32_t *>(c->pyr_peak.p);
    if (c->timing) HIP_TRY(hipEventRecord(c->ev0, s));
    TimingSuspended whole(c);           // (the events bracket the whole pass)
    // the coarsest level's displacement d_{L-1} and positions p_{L-1} (for L = 1: shift_out = shift)
    HIP_TRY(launch_pyr_step(call.d_xyuvav, N, call.off_u, call.off_v, call.d_shift, nullptr, call.R, levels - 1, true, sh, pos, s));
    SearchCall lv = call;               // level l: the points' positions on it, around sh, and the arg-max cells for the step to level l - 1
    lv.d_xyuvav = pos; lv.xy_stride = 2; lv.xy_col = 0; lv.off_u = lv.off_v = 0; lv.d_shift = sh; lv.npeaks = 0; lv.d_cand = nullptr; lv.d_peak = peak;
    for (int l = levels - 1; l >= 1; --l) {
        RC_TRY(plane_set(c, kernel, lc, l, planes));
        RC_TRY(launch_search(c, kernel, planes, lv));
        HIP_TRY(launch_pyr_step(call.d_xyuvav, N, call.off_u, call.off_v, nullptr, peak, call.R, l - 1, false, sh, pos, s));
    }
    SearchCall c0 = call;
    c0.d_shift = sh;
    RC_TRY(plane_set(c, kernel, lc, 0, planes));
    RC_TRY(launch_search(c, kernel, planes, c0));
    if (whole.was) { HIP_TRY(hipEventRecord(c->ev1, s)); c->timed = true; }
    return 0;
}

// The host entry of every search: the checks, the uploads, the device entry and the copies back.  What is staged follows from the
// output pointers: cand, surf, fb, and for a pyramid entry the shifts (shift_out may be null).
static int search_host(mimc3_ctx *c, const SearchRules &rules, const char *entry, const double *xyuvav, int32_t N, const int32_t offset[2],
                       const int32_t *shift, int32_t ocw, int32_t R, int32_t levels, int32_t npeaks, int32_t swap, int32_t mode, float *out,
                       float *cand, float *surf, float *fb, int32_t *shift_out)
{
    if (!offset) return fail(MIMC3_EINVAL, std::string(entry) + ": bad argument");
    SearchCall call = dev_call(entry, xyuvav, N, offset[0], offset[1], shift, ocw, R, npeaks, swap, mode, out, cand, surf, nullptr);
    call.host = true; call.levels = levels; call.d_fb = fb;
    RC_TRY(search_check(c, call, rules));
    RC_TRY(search_check_host(c, entry, xyuvav, N, offset, shift, ocw, R, rules.pyramid));
    const size_t n = (size_t)N, cand_bytes = sizeof(float) * 3 * (size_t)npeaks * n, fb_bytes = sizeof(float) * 4 * (size_t)(1 + npeaks) * n;
    const size_t surf_bytes = sizeof(float) * n * (size_t)((2 * R + 1) * (2 * R + 1));
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->xy.reserve(sizeof(double) * 6 * n));
    HIP_TRY(c->out.reserve(sizeof(float) * 8 * n));
    if (cand) HIP_TRY(c->full_cand.reserve(cand_bytes));
    if (surf) HIP_TRY(c->full_surf.reserve(surf_bytes));
    if (fb) HIP_TRY(c->fb_out.reserve(fb_bytes));
    if (rules.pyramid) HIP_TRY(c->pyr_sh.reserve(sizeof(int32_t) * 2 * n));
    RC_TRY(h2d_copy(c, c->xy.p, xyuvav, sizeof(double) * 6 * n));
    if (shift) {
        HIP_TRY(c->puv.reserve(sizeof(int32_t) * 2 * n));
        RC_TRY(h2d_copy(c, c->puv.p, shift, sizeof(int32_t) * 2 * n));
    }
    call.host = false;
    call.d_xyuvav = static_cast<const double *>(c->xy.p);
    call.d_shift = shift ? static_cast<const int32_t *>(c->puv.p) : nullptr;
    call.d_out = static_cast<float *>(c->out.p);
    call.d_cand = cand ? static_cast<float *>(c->full_cand.p) : nullptr;
    call.d_surf = surf ? static_cast<float *>(c->full_surf.p) : nullptr;
    call.d_fb = fb ? static_cast<float *>(c->fb_out.p) : nullptr;
    call.stream = c->stream;
    RC_TRY(rules.pyramid ? pyramid_dev(c, call, rules, static_cast<int32_t *>(c->pyr_sh.p))
           : rules.fb    ? full_fb_dev(c, call, rules)
                         : search_dev(c, call, rules));
    RC_TRY(d2h_copy(c, out, c->out.p, sizeof(float) * 8 * n));
    if (cand) RC_TRY(d2h_copy(c, cand, c->full_cand.p, cand_bytes));
    if (surf) RC_TRY(d2h_copy(c, surf, c->full_surf.p, surf_bytes));
    if (fb) RC_TRY(d2h_copy(c, fb, c->fb_out.p, fb_bytes));
    if (shift_out) RC_TRY(d2h_copy(c, shift_out, c->pyr_sh.p, sizeof(int32_t) * 2 * n));
    return 0;
}
}  // namespace mimc3

using namespace mimc3;

// ---------------------------------------------------------------------------------------------
// the public entries: each names itself, its rules and the arguments it has
// ---------------------------------------------------------------------------------------------
extern "C" int mimc3_match_ncc_full_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                        const int32_t *d_shift, int32_t ocw, int32_t R, int32_t swap, float *d_out, void *stream)
{
    return search_dev(c, dev_call("mimc3_match_ncc_full_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, 0, swap, 0, d_out, nullptr, nullptr, stream), kFull);
}

extern "C" int mimc3_match_ncc_full(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                    int32_t ocw, int32_t R, int32_t swap, float *out)
{
    return search_host(c, kFull, "mimc3_match_ncc_full", xyuvav, N, offset, shift, ocw, R, 0, 0, swap, 0, out, nullptr, nullptr, nullptr, nullptr);
}

// ... with the candidates of the best npeaks (1..8) local maxima of every point's surface
extern "C" int mimc3_match_ncc_full_multi_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                              const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, float *d_out,
                                              float *d_cand, void *stream)
{
    return search_dev(c, dev_call("mimc3_match_ncc_full_multi_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, swap, 0, d_out, d_cand, nullptr, stream),
                      kFullMulti);
}

extern "C" int mimc3_match_ncc_full_multi(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                          int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, float *out, float *cand)
{
    return search_host(c, kFullMulti, "mimc3_match_ncc_full_multi", xyuvav, N, offset, shift, ocw, R, 0, npeaks, swap, 0, out, cand, nullptr, nullptr, nullptr);
}

// ... on the planes the context matches on: an 8-bit pair as above, a scaled-integer pair (12-bit DN, a filtered 8-bit pair) through
// match_full_u16_kernel.hip on its u16 planes
extern "C" int mimc3_match_ncc_full_planes_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                               const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap,
                                               float *d_out, float *d_cand, void *stream)
{
    return search_dev(c, dev_call("mimc3_match_ncc_full_planes_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, swap, 0, d_out, d_cand, nullptr, stream),
                      kFullPlanes);
}

extern "C" int mimc3_match_ncc_full_planes(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                           int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, float *out, float *cand)
{
    return search_host(c, kFullPlanes, "mimc3_match_ncc_full_planes", xyuvav, N, offset, shift, ocw, R, 0, npeaks, swap, 0, out, cand, nullptr, nullptr, nullptr);
}

// ... and on an integral-f32 pair (16-bit DN and its filtered forms: every pixel x 1 or x 8 an integer in [0, 2^20)) through
// match_full_f32_kernel.hip on its f32 planes and 16-byte tables
extern "C" int mimc3_match_ncc_full_dn_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                           const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap,
                                           float *d_out, float *d_cand, void *stream)
{
    return search_dev(c, dev_call("mimc3_match_ncc_full_dn_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, swap, 0, d_out, d_cand, nullptr, stream),
                      kFullDn);
}

extern "C" int mimc3_match_ncc_full_dn(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                       int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, float *out, float *cand)
{
    return search_host(c, kFullDn, "mimc3_match_ncc_full_dn", xyuvav, N, offset, shift, ocw, R, 0, npeaks, swap, 0, out, cand, nullptr, nullptr, nullptr);
}

// ... on any f32 pair: mode 0 sends the classes above where mimc3_match_ncc_full_dn sends them and every other pair (non-integral
// pixels, NaN or negative nulls, values of 2^20 and above) through match_full_f32g_kernel.hip on its f32 planes (no tables); mode 1 sends
// any pair through that kernel.  Only that kernel serves the surfaces
extern "C" int mimc3_match_ncc_full_any_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                            const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode,
                                            float *d_out, float *d_cand, float *d_surf, void *stream)
{
    return search_dev(c, dev_call("mimc3_match_ncc_full_any_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, swap, mode, d_out, d_cand, d_surf, stream),
                      kFullAny);
}

extern "C" int mimc3_match_ncc_full_any(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                        int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode, float *out, float *cand,
                                        float *surf)
{
    return search_host(c, kFullAny, "mimc3_match_ncc_full_any", xyuvav, N, offset, shift, ocw, R, 0, npeaks, swap, mode, out, cand, surf, nullptr, nullptr);
}

// ... with the surfaces from whichever kernel runs: the class dispatch of mimc3_match_ncc_full_any(mode 0), surf mandatory -- the integer
// kernels in their surface-storing forms, the float kernel as ever
extern "C" int mimc3_match_ncc_full_surf_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                             const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, float *d_out,
                                             float *d_cand, float *d_surf, void *stream)
{
    return search_dev(c, dev_call("mimc3_match_ncc_full_surf_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, swap, 0, d_out, d_cand, d_surf, stream),
                      kFullSurf);
}

extern "C" int mimc3_match_ncc_full_surf(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                         int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, float *out, float *cand, float *surf)
{
    return search_host(c, kFullSurf, "mimc3_match_ncc_full_surf", xyuvav, N, offset, shift, ocw, R, 0, npeaks, swap, 0, out, cand, surf, nullptr, nullptr);
}

// ... at any chip half-width 1 .. 80: mode 0 at one of the six IS mimc3_match_ncc_full_any(mode 0); every other ocw, and all of mode 1,
// runs match_full_chip_kernel.hip (run-time ocw, the chip walked in bands) under mimc3_match_ncc_full_any's mode-1 definition
extern "C" int mimc3_full_chip_max_ocw(void) { return kFullChipMaxOcw; }
extern "C" int mimc3_full_chip_band_rows(int32_t ocw, int32_t R) { return full_chip_band_rows(ocw, R); }

extern "C" int mimc3_match_ncc_full_chip_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                             const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode,
                                             float *d_out, float *d_cand, float *d_surf, void *stream)
{
    return search_dev(c, dev_call("mimc3_match_ncc_full_chip_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, swap, mode, d_out, d_cand, d_surf, stream),
                      kFullChip);
}

extern "C" int mimc3_match_ncc_full_chip(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                         int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode, float *out, float *cand,
                                         float *surf)
{
    return search_host(c, kFullChip, "mimc3_match_ncc_full_chip", xyuvav, N, offset, shift, ocw, R, 0, npeaks, swap, mode, out, cand, surf, nullptr, nullptr);
}

// ... with the 8-bit pair on the matrix cores at every chip size (match_full_chip_u8_kernel.hip): mode 0 at one of the six is the class
// dispatch (surfaces as mimc3_match_ncc_full_surf serves them), at any other ocw an 8-bit pair runs the run-time-ocw matrix-core kernel and
// every other class the float kernel as above; mode 1 runs the matrix-core kernel at every ocw and takes 8-bit pairs only
extern "C" int mimc3_full_chip_class_layout(int32_t ocw, int32_t out[4])
{
    int l[4];
    if (!out || !full_chip_u8_layout(ocw, l)) return 0;
    for (int i = 0; i < 4; i++) out[i] = l[i];
    return 1;
}

extern "C" int mimc3_match_ncc_full_chip_class_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                                   const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode,
                                                   float *d_out, float *d_cand, float *d_surf, void *stream)
{
    return search_dev(c, dev_call("mimc3_match_ncc_full_chip_class_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, swap, mode, d_out, d_cand, d_surf, stream),
                      kFullChipClass);
}

extern "C" int mimc3_match_ncc_full_chip_class(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                               int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode, float *out, float *cand,
                                               float *surf)
{
    return search_host(c, kFullChipClass, "mimc3_match_ncc_full_chip_class", xyuvav, N, offset, shift, ocw, R, 0, npeaks, swap, mode, out, cand, surf, nullptr, nullptr);
}

// ... and with the scaled-integer pair on the matrix cores too (match_full_chip_u16_kernel.hip: q = 64 h + l, two 6-bit planes): mode 0 at one
// of the six is the class dispatch; at any other ocw an 8-bit pair runs the u8 matrix-core kernel, a scaled-integer pair the u16 one, every
// other class the float kernel; mode 1 runs the u16 matrix-core kernel at every ocw and takes 8-bit and scaled-integer pairs only
extern "C" int mimc3_full_chip_planes_layout(int32_t ocw, int32_t out[4])
{
    int l[4];
    if (!out || !full_chip_u16_layout(ocw, l)) return 0;
    for (int i = 0; i < 4; i++) out[i] = l[i];
    return 1;
}

extern "C" int mimc3_match_ncc_full_chip_planes_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                                    const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode,
                                                    float *d_out, float *d_cand, float *d_surf, void *stream)
{
    return search_dev(c, dev_call("mimc3_match_ncc_full_chip_planes_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, swap, mode, d_out, d_cand, d_surf, stream),
                      kFullChipPlanes);
}

extern "C" int mimc3_match_ncc_full_chip_planes(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                                int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode, float *out, float *cand,
                                                float *surf)
{
    return search_host(c, kFullChipPlanes, "mimc3_match_ncc_full_chip_planes", xyuvav, N, offset, shift, ocw, R, 0, npeaks, swap, mode, out, cand, surf, nullptr, nullptr);
}

// ... beyond +-15 px: mimc3_match_ncc_full_any in mode 1 with R up to mimc3_wide_max_radius(ocw).  R <= 15 IS that entry (the float
// kernel, its bytes); R >= 16 runs match_wide_kernel.hip on the same planes
extern "C" int mimc3_wide_max_radius(int32_t ocw) { return full_ocw_ok(ocw) ? wide_max_radius(ocw) : 0; }
extern "C" int mimc3_wide_lds_bytes(int32_t ocw, int32_t R) { return full_ocw_ok(ocw) ? wide_lds_bytes(ocw, R) : 0; }

extern "C" int mimc3_match_ncc_wide_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                        const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, float *d_out,
                                        float *d_cand, float *d_surf, void *stream)
{
    return search_dev(c, dev_call("mimc3_match_ncc_wide_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, swap, 1, d_out, d_cand, d_surf, stream), kWide);
}

extern "C" int mimc3_match_ncc_wide(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                    int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, float *out, float *cand, float *surf)
{
    return search_host(c, kWide, "mimc3_match_ncc_wide", xyuvav, N, offset, shift, ocw, R, 0, npeaks, swap, 1, out, cand, surf, nullptr, nullptr);
}

// ... and beyond +-15 px with the 8-bit pair on the matrix cores at every chip size (match_wide_u8_kernel.hip): R <= 15 IS
// mimc3_match_ncc_full_chip_class with the same mode; R >= 16 runs the matrix-core wide kernel on an 8-bit pair (mode 1 always; mode 0 where
// wide_mode0 names it, and wherever the float wide kernel does not take the call) and the float wide kernel on any other pair in mode 0
extern "C" int mimc3_wide_class_max_radius(int32_t ocw) { return wide_u8_max_radius(ocw); }
extern "C" int mimc3_wide_class_layout(int32_t ocw, int32_t R, int32_t out[4])
{
    int l[4];
    if (!out || !wide_u8_layout_query(ocw, R, l)) return 0;
    for (int i = 0; i < 4; i++) out[i] = l[i];
    return 1;
}

extern "C" int mimc3_match_ncc_wide_class_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                              const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode,
                                              float *d_out, float *d_cand, float *d_surf, void *stream)
{
    return search_dev(c, dev_call("mimc3_match_ncc_wide_class_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, swap, mode, d_out, d_cand, d_surf, stream),
                      kWideClass);
}

extern "C" int mimc3_match_ncc_wide_class(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                          int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode, float *out, float *cand,
                                          float *surf)
{
    return search_host(c, kWideClass, "mimc3_match_ncc_wide_class", xyuvav, N, offset, shift, ocw, R, 0, npeaks, swap, mode, out, cand, surf, nullptr, nullptr);
}

// ... and with the scaled-integer pair (12-bit DN, a filtered 8-bit pair) on the matrix cores as well (match_wide_u16_kernel.hip): R <= 15
// IS mimc3_match_ncc_full_chip_planes
extern "C" int mimc3_wide_planes_max_radius(int32_t ocw) { return wide_u16_max_radius(ocw); }
extern "C" int mimc3_wide_planes_layout(int32_t ocw, int32_t R, int32_t out[4])
{
    int l[4];
    if (!out || !wide_u16_layout_query(ocw, R, l)) return 0;
    for (int i = 0; i < 4; i++) out[i] = l[i];
    return 1;
}
extern "C" int mimc3_match_ncc_wide_planes_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                               const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode,
                                               float *d_out, float *d_cand, float *d_surf, void *stream)
{
    return search_dev(c, dev_call("mimc3_match_ncc_wide_planes_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, swap, mode, d_out, d_cand, d_surf, stream),
                      kWidePlanes);
}
extern "C" int mimc3_match_ncc_wide_planes(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                           int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode, float *out, float *cand,
                                           float *surf)
{
    return search_host(c, kWidePlanes, "mimc3_match_ncc_wide_planes", xyuvav, N, offset, shift, ocw, R, 0, npeaks, swap, mode, out, cand, surf, nullptr, nullptr);
}

// ... and beyond +-15 px on ANY pair at every chip size (match_wide_chip_kernel.hip): mode 1 is mimc3_match_ncc_full_any's definition on the
// run-time-ocw kernels (R <= 15 IS mimc3_match_ncc_full_chip(mode 1)); mode 0 runs the sibling that takes the call (wide_chip_kernel)
extern "C" int mimc3_wide_chip_max_radius(int32_t ocw) { return wide_chip_max_radius(ocw); }
extern "C" int mimc3_wide_chip_layout(int32_t ocw, int32_t R, int32_t out[5])
{
    int l[5];
    if (!out || !wide_chip_layout_query(ocw, R, l)) return 0;
    for (int i = 0; i < 5; i++) out[i] = l[i];
    return 1;
}
// the last_path of that entry for a pair class (0 8-bit, 1 scaled-integer, 2 integral f32, 3 any other), chip size, radius and mode; -1 outside the table
extern "C" int mimc3_wide_chip_path(int32_t pair_class, int32_t ocw, int32_t R, int32_t mode)
{
    SearchKernel kernel;
    if (pair_class < 0 || pair_class > 3 || !wide_chip_kernel(static_cast<PairClass>(pair_class), ocw, R, mode, kernel)) return -1;
    return 6 + (int)kernel;
}
extern "C" int mimc3_match_ncc_wide_chip_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                             const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode,
                                             float *d_out, float *d_cand, float *d_surf, void *stream)
{
    return search_dev(c, dev_call("mimc3_match_ncc_wide_chip_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, swap, mode, d_out, d_cand, d_surf, stream),
                      kWideChip);
}
extern "C" int mimc3_match_ncc_wide_chip(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                         int32_t ocw, int32_t R, int32_t npeaks, int32_t swap, int32_t mode, float *out, float *cand,
                                         float *surf)
{
    return search_host(c, kWideChip, "mimc3_match_ncc_wide_chip", xyuvav, N, offset, shift, ocw, R, 0, npeaks, swap, mode, out, cand, surf, nullptr, nullptr);
}

// ... and with forward-backward consistency
extern "C" int mimc3_match_ncc_full_fb_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                           const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, int32_t mode, float *d_out,
                                           float *d_cand, float *d_fb, void *stream)
{
    SearchCall call = dev_call("mimc3_match_ncc_full_fb_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, 0, mode, d_out, d_cand, nullptr, stream);
    call.d_fb = d_fb;
    return full_fb_dev(c, call, kFullFb);
}

extern "C" int mimc3_match_ncc_full_fb(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                       int32_t ocw, int32_t R, int32_t npeaks, int32_t mode, float *out, float *cand, float *fb)
{
    return search_host(c, kFullFb, "mimc3_match_ncc_full_fb", xyuvav, N, offset, shift, ocw, R, 0, npeaks, 0, mode, out, cand, nullptr, fb, nullptr);
}

extern "C" int mimc3_match_ncc_wide_fb_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                           const int32_t *d_shift, int32_t ocw, int32_t R, int32_t npeaks, float *d_out, float *d_cand,
                                           float *d_fb, void *stream)
{
    SearchCall call = dev_call("mimc3_match_ncc_wide_fb_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, 0, 1, d_out, d_cand, nullptr, stream);
    call.d_fb = d_fb;
    return full_fb_dev(c, call, kWideFb);
}

extern "C" int mimc3_match_ncc_wide_fb(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                       int32_t ocw, int32_t R, int32_t npeaks, float *out, float *cand, float *fb)
{
    return search_host(c, kWideFb, "mimc3_match_ncc_wide_fb", xyuvav, N, offset, shift, ocw, R, 0, npeaks, 0, 1, out, cand, nullptr, fb, nullptr);
}

// ... coarse to fine: on an 8-bit pair, on the classes of mimc3_match_ncc_full_dn, on any pair (with `mode`)
extern "C" int mimc3_match_ncc_pyramid_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                           const int32_t *d_shift, int32_t ocw, int32_t R, int32_t levels, int32_t swap, float *d_out,
                                           int32_t *d_shift_out, void *stream)
{
    SearchCall call = dev_call("mimc3_match_ncc_pyramid_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, 0, swap, 0, d_out, nullptr, nullptr, stream);
    call.levels = levels;
    return pyramid_dev(c, call, kPyramid, d_shift_out);
}

extern "C" int mimc3_match_ncc_pyramid_dn_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                              const int32_t *d_shift, int32_t ocw, int32_t R, int32_t levels, int32_t npeaks, int32_t swap,
                                              float *d_out, float *d_cand, int32_t *d_shift_out, void *stream)
{
    SearchCall call = dev_call("mimc3_match_ncc_pyramid_dn_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, swap, 0, d_out, d_cand, nullptr, stream);
    call.levels = levels;
    return pyramid_dev(c, call, kPyramidDn, d_shift_out);
}

extern "C" int mimc3_match_ncc_pyramid_any_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                               const int32_t *d_shift, int32_t ocw, int32_t R, int32_t levels, int32_t npeaks, int32_t swap,
                                               int32_t mode, float *d_out, float *d_cand, int32_t *d_shift_out, void *stream)
{
    SearchCall call = dev_call("mimc3_match_ncc_pyramid_any_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, swap, mode, d_out, d_cand, nullptr, stream);
    call.levels = levels;
    return pyramid_dev(c, call, kPyramidAny, d_shift_out);
}

extern "C" int mimc3_match_ncc_pyramid_chip_dev(mimc3_ctx *c, const double *d_xyuvav, int32_t N, int32_t off_u, int32_t off_v,
                                                const int32_t *d_shift, int32_t ocw, int32_t R, int32_t levels, int32_t npeaks, int32_t swap,
                                                int32_t mode, float *d_out, float *d_cand, int32_t *d_shift_out, void *stream)
{
    SearchCall call = dev_call("mimc3_match_ncc_pyramid_chip_dev", d_xyuvav, N, off_u, off_v, d_shift, ocw, R, npeaks, swap, mode, d_out, d_cand, nullptr, stream);
    call.levels = levels;
    return pyramid_dev(c, call, kPyramidChip, d_shift_out);
}

extern "C" int mimc3_match_ncc_pyramid(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                       int32_t ocw, int32_t R, int32_t levels, int32_t swap, float *out, int32_t *shift_out)
{
    return search_host(c, kPyramid, "mimc3_match_ncc_pyramid", xyuvav, N, offset, shift, ocw, R, levels, 0, swap, 0, out, nullptr, nullptr, nullptr, shift_out);
}

extern "C" int mimc3_match_ncc_pyramid_dn(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                          int32_t ocw, int32_t R, int32_t levels, int32_t npeaks, int32_t swap, float *out, float *cand,
                                          int32_t *shift_out)
{
    return search_host(c, kPyramidDn, "mimc3_match_ncc_pyramid_dn", xyuvav, N, offset, shift, ocw, R, levels, npeaks, swap, 0, out, cand, nullptr, nullptr, shift_out);
}

extern "C" int mimc3_match_ncc_pyramid_any(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                           int32_t ocw, int32_t R, int32_t levels, int32_t npeaks, int32_t swap, int32_t mode, float *out,
                                           float *cand, int32_t *shift_out)
{
    return search_host(c, kPyramidAny, "mimc3_match_ncc_pyramid_any", xyuvav, N, offset, shift, ocw, R, levels, npeaks, swap, mode, out, cand, nullptr, nullptr, shift_out);
}

// ... at any chip half-width 1 .. 80, on the run-time-ocw kernels (the matrix cores on 8-bit and scaled-integer pairs)
extern "C" int mimc3_match_ncc_pyramid_chip(mimc3_ctx *c, const double *xyuvav, int32_t N, const int32_t offset[2], const int32_t *shift,
                                            int32_t ocw, int32_t R, int32_t levels, int32_t npeaks, int32_t swap, int32_t mode, float *out,
                                            float *cand, int32_t *shift_out)
{
    return search_host(c, kPyramidChip, "mimc3_match_ncc_pyramid_chip", xyuvav, N, offset, shift, ocw, R, levels, npeaks, swap, mode, out, cand, nullptr, nullptr, shift_out);
}

// the last_path of that entry for a pair class (0 8-bit, 1 scaled-integer, 2 integral f32, 3 any other), chip size and mode; 0 outside the table
extern "C" int mimc3_pyramid_chip_path(int32_t pair_class, int32_t ocw, int32_t mode)
{
    SearchKernel kernel;
    if (pair_class < 0 || pair_class > 3 || !pyramid_chip_kernel(static_cast<PairClass>(pair_class), ocw, mode, kernel)) return 0;
    return 6 + (int)kernel;
}

// One level (1..4) of the current pair as pixel values, for tests of the reduction: the planes' interior of the level `kernel` reads.
// An integer class's planes are widened (u16 planes divided by 2^shift); f32 planes are copied as they are.
static int get_level(mimc3_ctx *c, SearchKernel kernel, int32_t level, float *out0, float *out1)
{
    PlaneSet pl;
    RC_TRY(plane_set(c, kernel, level, pl));
    const size_t es = kernel == Mx ? 1 : kernel == U16 ? 2 : 4, px = (size_t)pl.H * pl.W;
    std::vector<unsigned char> tmp(es < 4 ? es * px : 0);
    for (int k = 0; k < 2; k++) {
        float *out = k ? out1 : out0;
        void *dst = es == 4 ? static_cast<void *>(out) : static_cast<void *>(tmp.data());
        const unsigned char *src = static_cast<const unsigned char *>(k ? pl.p1 : pl.p0) + es * ((size_t)kU8Pad * pl.Wp + kU8Pad);
        HIP_TRY(hipMemcpy2DAsync(dst, es * pl.W, src, es * pl.Wp, es * pl.W, pl.H, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const float sc = 1.0f / (float)(1 << (k ? c->shift1 : c->shift0));
        if (kernel == Mx) for (size_t i = 0; i < px; i++) out[i] = (float)tmp[i];
        if (kernel == U16) for (size_t i = 0; i < px; i++) out[i] = (float)reinterpret_cast<const unsigned short *>(tmp.data())[i] * sc;
    }
    return 0;
}

// `any`: the FLOAT level, whatever the pair's class (mimc3_match_ncc_pyramid_any's levels); else the level of the pair's integer class
static int get_pyramid_level(mimc3_ctx *c, int32_t level, float *out0, float *out1, bool any, const std::string &en)
{
    if (!c || !out0 || !out1 || level < 1 || level > 4) return fail(MIMC3_EINVAL, en + ": bad argument");
    if (!c->d_i0 || !c->d_i1) return fail(MIMC3_ESTATE, en + ": images not set");
    if (c->child && (any || (!c->u8_ok && !c->u16_ok))) return fail(MIMC3_ESTATE, en + ": not on a chip-atlas context");
    PairClass cls = kFloat;
    if (!any) {
        RC_TRY(check_class(c, kIntegralF32, en));
        RC_TRY(pair_class(c, cls));
    }
    if ((c->H >> level) < 1 || (c->W >> level) < 1) return fail(MIMC3_EINVAL, en + ": level " + std::to_string(level) + " is empty");
    HIP_TRY(hipSetDevice(c->device));
    return get_level(c, cls == kU8 ? Mx : cls == kScaledInt ? U16 : cls == kIntegralF32 ? F32i : F32g, level, out0, out1);
}

extern "C" int mimc3_ctx_get_pyramid_level(mimc3_ctx *c, int32_t level, float *out0, float *out1)
{
    return get_pyramid_level(c, level, out0, out1, false, "mimc3_ctx_get_pyramid_level");
}

extern "C" int mimc3_ctx_get_pyramid_level_any(mimc3_ctx *c, int32_t level, float *out0, float *out1)
{
    return get_pyramid_level(c, level, out0, out1, true, "mimc3_ctx_get_pyramid_level_any");
}
