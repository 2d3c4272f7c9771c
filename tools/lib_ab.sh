#!/bin/bash
# A/B of two builds of the library on the bench's pass, alternating, in one call (boxes differ by ~10 %: never compare
# across calls).   bash tools/lib_ab.sh libtdaeeg_prev.so libtdaeeg.so [bench flags]
# An argument that is a directory is a whole built tree (an earlier commit beside this one, for a library whose exported
# symbols differ from what this tree's _lib.py binds): its own bench.py runs there with its own library.
# Each run is a process of its own under its own time limit; the first run that fails ends the script.  Every line ends with
# the sha256 of the run's result rows (bench.py --dump-outputs), so "the same bytes" is read off the lines.
A=$1; B=$2; shift 2
OUT=$(mktemp -d) || exit 1
trap 'rm -rf "$OUT"' EXIT
for rep in 1 2 3; do
    for l in $A $B; do
        rm -f "$OUT/rows/rows.npy"
        if [ -d "$l" ]; then
            (cd "$l" && timeout -k 10 200 python bench.py --no-cpu --no-extras --steps 40 --dump-outputs "$OUT/rows" "$@") > "$OUT/lab.json" 2> "$OUT/lab.err"
        else
            TDA_LIB=$l timeout -k 10 200 python bench.py --no-cpu --no-extras --steps 40 --dump-outputs "$OUT/rows" "$@" > "$OUT/lab.json" 2> "$OUT/lab.err"
        fi || { echo "$l failed"; tail -3 "$OUT/lab.err"; exit 1; }
        python -c "
import hashlib,json;d=json.loads(open('$OUT/lab.json').read().strip().splitlines()[-1]);print($rep,'$l',round(d['value']),round(d['ms_per_step'],4),'ms',hashlib.sha256(open('$OUT/rows/rows.npy','rb').read()).hexdigest()[:16])"
    done
done
