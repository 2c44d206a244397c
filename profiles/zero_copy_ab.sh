# The downlink slot pipeline under each NRPHY_DL_SLOT_ZERO_COPY mode: its parity tests, then its latency.  Every GPU step runs under
# a limit, and the first one that fails ends the script: nothing more starts on the card after it.  GPU box, repository root.
set -u -o pipefail
for m in 0 1 2 3; do
  echo "== NRPHY_DL_SLOT_ZERO_COPY=$m"
  NRPHY_DL_SLOT_ZERO_COPY=$m timeout -k 10 300 python -m pytest tests/test_gpu_parity.py -x -q -m gpu -k "dl_slot" 2>&1 | tail -1 || exit $?
  NRPHY_DL_SLOT_ZERO_COPY=$m timeout -k 10 200 python3 -c "
import sys; sys.path.insert(0, 'profiles'); sys.path.insert(0, 'tests')
import shim_latency as s
s.dl_slot_pipeline(depths=(1, 4, 8), check=True)
" 2>&1 | grep "slot pipeline" | sed 's/; PCIe per slot.*host time/; host time/' || exit $?
done
