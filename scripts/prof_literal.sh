# usage (GPU box, repo root): bash scripts/prof_literal.sh <tag> [S N W reps]  -> ${OUT}/<tag>_kernel_stats.csv (rocprofv3 kernel trace of the literal route, conv = rocfft)
cd ${GRAFT_REPO_ROOT:-.}
TAG=$1; shift
OUT=${JOXSZ_PROFILE_OUT:-profile_out}
mkdir -p ${OUT}
export TMPDIR=/tmp
rm -rf ${OUT}/prof_${TAG}
rocprofv3 --kernel-trace -d ${OUT}/prof_${TAG} -- python3 scripts/literal_prof.py "$@" > ${OUT}/${TAG}_run.log 2>&1
tail -2 ${OUT}/${TAG}_run.log
DB=$(ls ${OUT}/prof_${TAG}/*/*results.db | head -1)
test -n "$DB" && python3 scripts/kstats.py $DB ${OUT}/${TAG}_kernel_stats.csv
rm -rf ${OUT}/prof_${TAG}
