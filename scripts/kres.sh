#!/bin/bash
# Register / scratch / occupancy of the qp_step instantiations (and the line-search, KKT and sensitivity kernels), with the library's own compile flags and
# sources (build.FLAGS, build.SOURCES; developer tool, no GPU).  Extra arguments (e.g. -DQSP_MIN_WAVES=2)
# are appended.
cd "$(dirname "$0")/.." || exit 1
FLAGS=$(python3 -c "from uclv_qs_pushing_matlab_amd.build import FLAGS; print(' '.join(f for f in FLAGS if f not in ('-shared', '-fPIC')))")
SOURCES=$(python3 -c "from uclv_qs_pushing_matlab_amd.build import SOURCES; print(' '.join(SOURCES))")
for f in $SOURCES; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 $FLAGS -I include "$@" \
    -c uclv_qs_pushing_matlab_amd/csrc/$f -o /tmp/kres.o -Rpass-analysis=kernel-resource-usage 2>&1
done |
  sed -n -e 's/ \[-Rpass.*//' -e 's/.*remark: *//p' |
  awk '/^Function Name:/ { if (row != "") print row; row = ($0 ~ /_ZN3qsp1(4qp_step|5sqp_loop|5merit_ls|4kkt_nlp|3kkt_qp|5sens_lin|6sens_walk|9sens_walk_qp)/) ? $0 : "" ; next }
       row != "" && /^(VGPRs:|AGPRs:|ScratchSize|Occupancy)/ { row = row "\t" $0 }
       END { if (row != "") print row }'
