#!/bin/bash
# test_env_matrix.sh [SWITCH=value ...] -- GPU box: tests/test_gpu_parity.py under every launch-form switch of the library (each switch
# selects other kernel instances for the same calls; results must not depend on it), or under the ones named.  About two minutes per
# line, each under a time limit of its own; the first configuration that fails or runs out of time ends the script with its status:
# nothing more is started on the card after it.
# (MBX_NO_LDS_RESIDENT is not in the list: the full-shape tests assert the default instances BY NAME, which that switch replaces on purpose.)
cd "$(dirname "$0")/.." || exit 1
configs=("$@")
if [ ${#configs[@]} -eq 0 ]; then
  configs=("MBX_FUSE_ONE=0" "MBX_FUSE_ONE=1" "MBX_SLICE_OWN=0" "MBX_SLICE=0" "MBX_SLICE_GROUPS=2" "MBX_NO_RES1=1" "MBX_FRONT_LEAD=64" "MBX_NO_REVERSE=1")
fi
for e in "${configs[@]}"; do
  echo "== $e"
  timeout -k 10 600 env "$e" python -m pytest tests/test_gpu_parity.py -m gpu -x -q --deselect tests/test_gpu_parity.py::test_bench_default_line_keeps_its_contract
  rc=$?
  if [ "$rc" -ne 0 ]; then
    echo "== FAILED under $e (exit status $rc)" >&2
    exit "$rc"
  fi
done
echo "== all configurations passed"
