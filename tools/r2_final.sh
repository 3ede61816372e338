# round 2, final GPU call: parity suite, smoke, the default bench line, then the profile pass (tools/r2_callB.sh)
set -e
TAG=${TAG:-r2g}
O=${OUT:?OUT must name the folder for the outputs}
mkdir -p $O
timeout -k 10 850 python -m pytest tests -x -q -m gpu > $O/${TAG}_pytest.log 2>&1 || { tail -30 $O/${TAG}_pytest.log; exit 1; }
tail -2 $O/${TAG}_pytest.log
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')"
python bench.py --full > $O/${TAG}_bench_default.json 2> $O/${TAG}_bench_default.err
tail -c 600 $O/${TAG}_bench_default.json
TAG=$TAG bash tools/r2_callB.sh > $O/${TAG}_callB.log 2>&1
cp $O/${TAG}_bench_default.json $O/$TAG/bench_default.json
tail -5 $O/${TAG}_callB.log
