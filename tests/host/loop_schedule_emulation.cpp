// CPU check of the fast loops' schedules (csrc/loop_schedule.h, the header the engines and pnp_get_plan run by): the plan of
// each case and the parts it runs, as the engines enqueue them (engine_host.h, run_parts).
//   loop_schedule_emulation <case>...      case = kind:B:queues:mixed:chunk[:chunk_queues[:slice_queues]]
//   kind: f256 (two-launch 256x256), s32 / s64 (split chain in float / double), f512, slice
//   out : one line per case, "queues chunk launches | first,count,queue[m] ..." (m: the part takes the mixed launches)
#include "../../pnp_admm_cnc_mri_amd/csrc/loop_schedule.h"

#include <stdio.h>
#include <string.h>

using namespace pnp;

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        char kind[8] = {0};
        int B = 0;
        FusedSchedule sch;
        if (sscanf(argv[a], "%7[^:]:%d:%d:%d:%d:%d:%d", kind, &B, &sch.queues, &sch.mixed, &sch.chunk, &sch.chunk_queues,
                   &sch.slice_queues) < 5) {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        LoopPlan p;
        if (!strcmp(kind, "f256"))       p = plan_fused256(B, sch);
        else if (!strcmp(kind, "s32"))   p = plan_chunked(B, sch, Chunked::split_f32);
        else if (!strcmp(kind, "s64"))   p = plan_chunked(B, sch, Chunked::split_f64);
        else if (!strcmp(kind, "f512"))  p = plan_chunked(B, sch, Chunked::fused512);
        else if (!strcmp(kind, "slice")) p = plan_slice(B, sch);
        else { fprintf(stderr, "bad kind %s\n", kind); return 2; }
        printf("%d %d %d |", p.queues, p.chunk, p.launches);
        int next = 0;
        for (int i = 0; i < p.parts; ++i) {
            const Part q = plan_part(p, B, i);
            // the parts tile the batch in order, each on one of the plan's queues
            if (q.first != next || q.count <= 0 || q.queue < 0 || q.queue >= p.queues || q.queue >= kMaxQueues) {
                fprintf(stderr, "%s: part %d = (%d, %d, %d) does not follow on slice %d\n", argv[a], i, q.first, q.count, q.queue, next);
                return 1;
            }
            next += q.count;
            printf(" %d,%d,%d%s", q.first, q.count, q.queue, takes_mixed(p, q) ? "m" : "");
        }
        if (next != B) { fprintf(stderr, "%s: parts cover %d of %d slices\n", argv[a], next, B); return 1; }
        printf("\n");
    }
    return 0;
}
