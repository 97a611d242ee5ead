#!/bin/bash
# N = 4 and N = 8 rehearsals of bench.py on ONE GPU (gloo ranks sharing cuda:0):
# checks the multi-rank code paths (partition, hybrid plan, exchanges, parity
# checks) at the full C4 size; gloo moves rows through host memory, so the
# times say nothing about RCCL / xGMI.  Then the corrected halo probe.
# Logs go to $DGLMI_OUT (default build/out).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
out=${DGLMI_OUT:-build/out}
mkdir -p "$out"
export TMPDIR=/tmp
for N in ${NS:-4 8}; do
  DGLMI_BENCH_TRACE="$out"/trace_n$N timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node $N --master-addr 127.0.0.1 --master-port 2955$N bench.py --full --gpus $N --dist-backend gloo --same-device --steps 2 --warmup 1 --edges-per-gpu 5000000 --scale 19 ${C4ARGS:-} > "$out"/rehearse_n$N.json 2> "$out"/rehearse_n$N.err
  rc=$?; echo "N=$N rc=$rc"; tail -c 1500 "$out"/rehearse_n$N.json; grep -v Gloo "$out"/rehearse_n$N.err | tail -4
  [ $rc -eq 0 ] || exit $rc
done
timeout -k 10 300 python -u scripts/halo_probe.py > "$out"/halo_probe.log 2>&1
rc=$?; echo "halo rc=$rc"; tail -3 "$out"/halo_probe.log
exit $rc
