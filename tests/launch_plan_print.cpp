// Prints plan_launch() of quadruped_landing_amd/csrc/qln_launch_plan.h for the requests on standard input, one per line:
//   nb N jac_format kt_max c vals f grad prefer_latency variant prefetch_ahead prefetch_mask pad_lds
// Host code only (hipcc --offload-host-only); tests/test_launch_plan_host.py builds and runs it without a device.
#include <cstdio>

#include "../quadruped_landing_amd/csrc/qln_launch_plan.h"

int main() {
    int nb, N, fmt, kt, c, vals, f, grad, lat, variant, ahead, mask;
    unsigned pad;
    while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %u", &nb, &N, &fmt, &kt, &c, &vals, &f, &grad, &lat, &variant, &ahead, &mask,
                      &pad) == 13) {
        qln::LaunchRequest r;
        r.nb = nb, r.N = N, r.jac_format = fmt, r.kt_max = kt;
        r.c = c != 0, r.vals = vals != 0, r.f = f != 0, r.grad = grad != 0, r.prefer_latency = lat != 0;
        r.variant = variant, r.prefetch_ahead = ahead, r.prefetch_mask = mask, r.pad_lds = pad;
        const qln::LaunchPlan p = qln::plan_launch(r);
        std::printf("<%d,%d,%d,%d,%d,%d,%d,%d,%d> wg=%d lds=%u ahead=%u what=%u flags=%u\n", p.T, p.KC, p.W, (int)p.with_c, (int)p.with_j,
                    (int)p.nnz, (int)p.split, (int)p.stream, (int)p.with_f, p.workgroups, p.lds_bytes, p.prefetch_ahead,
                    p.prefetch_what >> 29, qln::kernel_flags(p, true));
    }
    return 0;
}
