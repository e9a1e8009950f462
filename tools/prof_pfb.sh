#!/bin/bash
# rocprofv3 of the polyphase + FFT channelizer, one process per shape (two K classes share a kernel instantiation, so one trace per shape):
# a kernel trace, then - in runs of their own - FETCH_SIZE and WRITE_SIZE.   tools/prof_pfb.sh <tag> [outdir [oversample]] -> <outdir>/prof_<tag>/summary_pfb.txt (default outdir: build/, untracked; oversample 2 or 4 profiles pfb_oversampled_kernel)
TAG=${1:-r}
ROOT=$(pwd)
OUT=${2:-$ROOT/build}/prof_$TAG
R=${3:-1}
mkdir -p "$OUT"; rm -rf "$OUT/pfb"
export TMPDIR=/tmp
cd /tmp
for shape in "64 1024" "256 4096" "512 8192" "1024 16384" "2048 32768" "4096 65536"; do
    set -- $shape
    timeout -k 10 120 rocprofv3 --kernel-trace --stats -d "$OUT/pfb/kt_$1" -o p -- python $ROOT/tools/run_pfb_channelizer.py $1 $2 20 $R > /dev/null 2>&1 || { echo "kernel trace K=$1 failed"; exit 1; }
    timeout -k 10 120 rocprofv3 --pmc FETCH_SIZE -d "$OUT/pfb/fetch_$1" -o p -- python $ROOT/tools/run_pfb_channelizer.py $1 $2 3 $R > /dev/null 2>&1 || { echo "FETCH_SIZE K=$1 failed"; exit 1; }
    timeout -k 10 120 rocprofv3 --pmc WRITE_SIZE -d "$OUT/pfb/write_$1" -o p -- python $ROOT/tools/run_pfb_channelizer.py $1 $2 3 $R > /dev/null 2>&1 || { echo "WRITE_SIZE K=$1 failed"; exit 1; }
done
cd "$ROOT"
python profiles/summarize_rocpd.py "$OUT/pfb" pfb_ --last 10 > "$OUT/summary_pfb.txt" 2>&1
find "$OUT/pfb" -name "*.db" -delete
grep -c pfb_ "$OUT/summary_pfb.txt"
