# A/B of two builds on ONE GPU box (box-to-box spread is ~2 %): clipcap_amd/libclipcap_hip_old.so (e.g. built from `git archive HEAD`
# with `make OUT=.../libclipcap_hip_old.so`) against the current library; alternates them three times.  Prints ms_per_step per run, and
# tokens/s beside it for "--mode decode".  Every run has its own time limit (AB_TIMEOUT seconds, default 600); the first run that fails
# or times out ends the script (with the current library back in place): nothing more is started on a GPU that may have faulted.
# usage (on the GPU box, from the repository root): bash tools/ab_bench.sh ["--config 2" "--config 3" "--mode mapper" "--mode decode" ...]
set -o pipefail
cd ${GRAFT_REPO_ROOT:-.}
cp clipcap_amd/libclipcap_hip.so /tmp/new.so; cp clipcap_amd/libclipcap_hip_old.so /tmp/old.so || exit 1
[ $# -eq 0 ] && set -- "--config 2" "--config 3"
for r in 1 2 3; do
  for v in old new; do
    cp /tmp/$v.so clipcap_amd/libclipcap_hip.so
    line="$v:"
    for a in "$@"; do
      out=$(timeout -k 10 ${AB_TIMEOUT:-600} python bench.py $a --no-cpu-baseline --no-sub-benches --no-roofline-pass --steps 60 --warmup 10 2>&1 | tail -1)
      rc=$?
      ms=$(echo "$out" | grep -o '"ms_per_step": [0-9.]*' | head -1 | cut -d' ' -f2)
      if [ $rc -ne 0 ] || [ -z "$ms" ]; then echo "$line  [$a] FAILED (status $rc): $out"; cp /tmp/new.so clipcap_amd/libclipcap_hip.so; exit 1; fi
      tok=$(echo "$out" | grep -o '"value": [0-9.]*, "unit": "tokens/s"' | head -1 | cut -d' ' -f2 | tr -d ,)
      line="$line  [$a] $ms${tok:+ ms, $tok tok/s}"
    done
    echo "$line"
  done
done
cp /tmp/new.so clipcap_amd/libclipcap_hip.so
