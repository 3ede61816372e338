# round 4, call 27: Canberra lists seeded with the first 256 references of their split before the count starts
O=$PWD/gpurun_out/${TAG:-r4c28}; mkdir -p $O

for so in tools/ab/seed512.so tools/ab/seed768.so tools/ab/seed1024.so tools/ab/seed1536.so tools/ab/seed512.so; do
  tag=$( [ -z "$so" ] && echo product || basename $so .so )
  for shape in "100000 100000" "1000000 1000000" "30000 60000"; do
    NABO_KNN_SO=$so timeout -k 10 200 python bench.py --full --metric canberra --targets ${shape% *} --refs ${shape#* } --steps 3 --warmup 1 --no-extras --no-cpu-baseline > $O/cb_${tag}_$(echo $shape | tr ' ' 'x').json 2>> $O/err.txt
    python - <<PY
import json
d=json.loads(open("$O/cb_${tag}_$(echo $shape | tr ' ' 'x').json").read().strip().splitlines()[-1]); print("$tag $shape ms/step %.2f kernel %.2f"%(d["ms_per_step"], d["roofline"]["kernel_ms"]), d["sampled_rows_equal_oracle"])
PY
  done
done
