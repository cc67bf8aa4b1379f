// Host program for tests/test_host_flow_sched.py: prints the pass schedule of csrc/i2v_flow_sched.h, one line per link, for
// n_flows in {1, 2, 3, 20} x both directions x the eight (ActNorm, activation, Shuffle) switch combinations = 64 schedules.
#include "i2v_flow_sched.h"

#include <cstdio>

int main() {
    const int nfs[4] = {1, 2, 3, 20};
    for (int nf : nfs)
        for (int rev = 0; rev < 2; ++rev)
            for (int m = 0; m < 8; ++m) {
                const bool an = m & 4, act = m & 2, sh = m & 1;
                printf("schedule nf=%d dir=%s an=%d act=%d shuf=%d\n", nf, rev ? "rev" : "fwd", an, act, sh);
                for (const i2v::FlowLink& k : i2v::flow_schedule(nf, rev != 0, an, act, sh))
                    printf("link step=%d shuf=%d an=%d lrelu=%d swap=%d next=%d\n", k.step, k.shuf_block, k.an_block, k.lrelu ? 1 : 0,
                           k.swap ? 1 : 0, k.next_step);
            }
    // the two loader helpers, so that a change of the naming rule or the 'cond' rule shows up here as well
    printf("key %s %s\n", i2v::flow_linear_key(0, 0, 0, 0).c_str(), i2v::flow_linear_key(19, 1, 1, 3).c_str());
    printf("cond");
    for (int control = 0; control < 3; ++control)
        for (int fl = 0; fl < 6; ++fl) printf(" %d", i2v::flow_block_cond(control, fl) ? 1 : 0);
    printf("\n");
    return 0;
}
