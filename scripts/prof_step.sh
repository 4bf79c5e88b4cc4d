# usage (on the GPU box, repo root): bash scripts/prof_step.sh <tag> [bench args]  -> ${OUT}/<tag>_bench.json, ${OUT}/<tag>_kernel_stats.csv
cd ${GRAFT_REPO_ROOT:-.}
TAG=$1; shift
OUT=${JOXSZ_PROFILE_OUT:-profile_out}
mkdir -p ${OUT}
export TMPDIR=/tmp
python bench.py --full --no-cpu --steps 100 --warmup 5 --regions 25 "$@" > ${OUT}/${TAG}_bench.json 2> ${OUT}/${TAG}_bench.err || { tail -5 ${OUT}/${TAG}_bench.err; exit 1; }
python -c "import json; j=json.load(open('${OUT}/${TAG}_bench.json')); print('value %.0f  ms/step %.4f' % (j['value'], j['ms_per_step'])); print(j['stage_ms_per_step'])"
rm -rf ${OUT}/prof_${TAG}
rocprofv3 --kernel-trace -d ${OUT}/prof_${TAG} -- python3 bench.py --full --no-cpu --no-full-map --no-f32 --no-other-configs --no-other-routes --no-host-pointer --steps 100 --warmup 5 --regions 5 "$@" > /dev/null 2>&1
DB=$(ls ${OUT}/prof_${TAG}/*/*results.db | head -1)
python scripts/kstats.py $DB ${OUT}/${TAG}_kernel_stats.csv
rm -rf ${OUT}/prof_${TAG}
