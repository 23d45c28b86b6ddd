cd "$(dirname "$0")/.."; O=${OUT:-out/tile_policy_1}; mkdir -p $O
timeout -k 10 300 python3 bench.py --full --no-cpu-baseline > $O/full.json 2>/dev/null
python3 -c "
import json; d=json.load(open('$O/full.json')); print('headline', d['value'], 'tile_policy_1 section', d['tile_policy_1'])"
timeout -k 10 200 python3 bench.py --full --no-extras --no-cpu-baseline --no-verify --lanes 2 --tile-policy 1 > $O/p1.json 2>/dev/null
python3 -c "
import json; d=json.load(open('$O/p1.json')); print('standalone policy 1', d['value'], d['value_windows'])"
