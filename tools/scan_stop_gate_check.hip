// Stand-alone check of hops_host.h::scan_stop_gate -- the host decision "may this launch take the stopping hop kernel" and its
// threshold arithmetic -- for a sanitizer build of the HOST code (no kernel is launched, no GPU is needed):
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/scan_stop_gate_check.hip -o /tmp/scan_stop_gate_check && /tmp/scan_stop_gate_check
#include "../q-mann_amd/csrc/hops_mid.h"
#include "../q-mann_amd/csrc/hops_host.h"
#include <math.h>
#include <stdio.h>

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static HopArgs args(uint32_t iwl, uint32_t frac, uint32_t n_hop = 3)
{
    HopArgs a{};
    a.n_hop = n_hop; a.D = a.Dp = 128; a.softmax_base = QMANN_SOFTMAX_EXP;
    for (uint32_t h = 0; h < n_hop; h++) a.act[h] = a.w[h] = a.att[h] = QFmt{iwl, frac};
    a.bin = QFmt{iwl, frac};
    return a;
}

int main()
{
    // Q2.5: 32 e^(127/32) (1 + 2^-6) = 1 719.9 rows
    EXPECT(scan_stop_gate(args(2, 5), 1720) && scan_stop_gate(args(2, 5), 10000) && !scan_stop_gate(args(2, 5), 1719));
    // Q5.2 (4 e^31.75 rows) and Q7.0 never; Q0.7: 128 e^(127/128) (1 + 2^-6) = 350.6
    EXPECT(!scan_stop_gate(args(5, 2), 10000) && !scan_stop_gate(args(5, 2), 0xFFFFFFFFu) && !scan_stop_gate(args(7, 0), 0xFFFFFFFFu));
    EXPECT(scan_stop_gate(args(0, 7), 351) && !scan_stop_gate(args(0, 7), 350));
    // one hop that can stop is enough
    { HopArgs a = args(5, 2); a.att[2] = a.act[2] = QFmt{2, 5}; EXPECT(scan_stop_gate(a, 2000)); a.n_hop = 2; EXPECT(!scan_stop_gate(a, 2000)); }
    // any tap, another base, the shift softmax: the plain kernel
    float f = 0; int32_t i = 0;
    { HopArgs a = args(2, 5); a.tap_codes = &i; EXPECT(!scan_stop_gate(a, 10000)); }
    { HopArgs a = args(2, 5); a.tap_scores = &f; EXPECT(!scan_stop_gate(a, 10000)); }
    { HopArgs a = args(2, 5); a.tap_probs = &f; EXPECT(!scan_stop_gate(a, 10000)); }
    { HopArgs a = args(2, 5); a.tap_o = &f; EXPECT(!scan_stop_gate(a, 10000)); }
    { HopArgs a = args(2, 5); a.tap_u = &f; EXPECT(!scan_stop_gate(a, 10000)); }
    { HopArgs a = args(2, 5); a.softmax_base = QMANN_SOFTMAX_POW2; EXPECT(!scan_stop_gate(a, 10000)); a.softmax_base = QMANN_SOFTMAX_EXP_PLAN; EXPECT(!scan_stop_gate(a, 10000)); }
    { HopArgs a = args(2, 5); a.softmax_shift = 1; EXPECT(!scan_stop_gate(a, 10000)); }
    // the scale layer: either sign halves Xb at 0.5 (32 e^1.984 (1 + 2^-6) = 236.4 rows); 0 leaves e^0 per row; NaN and the infinities never open
    for (float s : {0.5f, -0.5f}) { HopArgs a = args(2, 5); a.en_att_scale = 1; for (float &x : a.att_scale) x = s; EXPECT(scan_stop_gate(a, 237) && !scan_stop_gate(a, 236)); }
    { HopArgs a = args(2, 5); a.en_att_scale = 1; EXPECT(scan_stop_gate(a, 33) && !scan_stop_gate(a, 32)); }
    for (float s : {NAN, INFINITY, -INFINITY, 3.0e38f, -3.0e38f}) { HopArgs a = args(2, 5); a.en_att_scale = 1; for (float &x : a.att_scale) x = s; EXPECT(!scan_stop_gate(a, 0xFFFFFFFFu)); }
    { HopArgs a = args(2, 5); for (float &x : a.att_scale) x = NAN; EXPECT(scan_stop_gate(a, 1720)); }      // (scale layer off: its words are not read)
    // every byte format, both ends of the slot range: no shift or conversion out of range
    unsigned open = 0;
    for (uint32_t iwl = 0; iwl <= 7; iwl++)
        for (uint32_t frac = 0; iwl + frac <= 7; frac++)
            if (iwl + frac >= 1)
                for (uint32_t n : {0u, 1u, 257u, 10000u, 0xFFFFFFFFu}) open += scan_stop_gate(args(iwl, frac, QMANN_MAX_HOP), n);
    printf("scan_stop_gate: %d failures; %u of the format x size grid open\n", failures, open);
    return failures ? 1 : 0;
}
