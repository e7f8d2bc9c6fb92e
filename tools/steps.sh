# Sourced by the scripts that run on the GPU box (prof_all.sh, ab.sh, wgx_abl.sh).
#   step SECONDS LOG CMD...   runs CMD under `timeout -k 10 SECONDS` with stderr appended to LOG (stdout is the caller's to redirect)
#                             and reports the wall time it took on stderr.
# On any non-zero status (124 = the time limit) it prints the end of LOG and EXITS THE SCRIPT with that status, so nothing more is
# started on a card after a fault, an abort or a hang.
# OUT is where those scripts write: $HRN_OUT, or scratch/out in the repository (scratch/ is not tracked).
OUT=${HRN_OUT:-$(dirname "${BASH_SOURCE[0]}")/../scratch/out}
OUT=$(mkdir -p "$OUT" && cd "$OUT" && pwd)          # absolute: prof_all.sh changes directory

step() {
  local limit=$1 log=$2 status=0 t0=$SECONDS
  shift 2
  timeout -k 10 "$limit" "$@" 2>> "$log" || status=$?
  if [ $status -ne 0 ]; then
    echo "step failed with status $status after $((SECONDS - t0)) s (limit $limit s): $*" >&2
    tail -5 "$log" >&2
    exit $status
  fi
  echo "step took $((SECONDS - t0)) s of $limit s: $*" >&2
}
