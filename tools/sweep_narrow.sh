#!/bin/bash
# tools/sweep_narrow.sh: tools/sweep_narrow_threads.py for every library in LIBS (default: the build)
R=${GRAFT_REPO_ROOT:-/root/repo}
mkdir -p $R/gpurun_out/r6m; echo "cpus $(nproc)  cgroup cpu.max $(cat /sys/fs/cgroup/cpu.max 2>/dev/null)"
for LIB in ${LIBS:-$R/nanomod_amd/libnanomod_hip.so}; do
  NMOD_HIP_LIB=$LIB python3 $R/tools/sweep_narrow_threads.py "$@" 2>&1 | tee -a $R/gpurun_out/r6m/sweep_narrow.txt
done
