cd "$(dirname "$0")/.."; O=${OUT:-out/lanes23}; mkdir -p $O
for i in 1 2 3; do for l in 2 3; do
timeout -k 10 200 python3 bench.py --full --no-extras --no-cpu-baseline --no-verify --lanes $l > $O/l${l}_$i.json 2>/dev/null
python3 -c "
import json; d=json.load(open('$O/l${l}_$i.json')); print('lanes $l run $i', d['value'], d['value_windows']['min'], d['value_windows']['median'], d['value_windows']['max'])"
done; done
