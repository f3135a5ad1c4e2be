#!/bin/bash
# Round-3 closing sequence on the shipped build: GPU tests, smoke, counter collection (stamps profiles/latest_*.json), bench line.
set -u
TAG=${1:-r03n}
cd "$GRAFT_REPO_ROOT"; export TMPDIR=/tmp; O=gpurun_out; mkdir -p $O
( time timeout -k 10 900 python -m pytest tests -m gpu -x -q ) > $O/${TAG}_pytest.log 2>&1; rc=$?; grep -E "passed|failed|error" $O/${TAG}_pytest.log | tail -2; [ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python __graft_entry__.py smoke 2>&1 | grep -v amdgpu | tail -1
timeout -k 10 1000 python tools/collect_profiles.py $TAG headline c3 c5 > $O/${TAG}_collect.log 2>&1; echo "collect rc=$?"
cp $O/profiles_$TAG/latest_pmc.json profiles/latest_pmc.json; cp $O/profiles_$TAG/latest_other_configs.json profiles/latest_other_configs.json
timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err; echo "bench rc=$?"; cut -c1-200 $O/${TAG}_bench.json
