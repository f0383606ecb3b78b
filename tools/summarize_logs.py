"""Table of the training runs under a logs directory: examples/summarize_logs.py restated (pandas
``.loc`` instead of the removed ``.ix``; the logs directory is an argument).

    python tools/summarize_logs.py logs

One row per run directory (params.yaml + log of tools/train.py), newest first: the row of the log
entry with the best ``validation/main/map``, the run's settings and, when tools/evaluate.py
--log-dir has been run on it, the map of snapshot_model.npz.eval_result.yaml.  Directories
without params.yaml are listed as ignored.  A ``validation/main/bbox/map`` column (box AP, tools/
train.py --eval-bbox) is shown when some run's log has it, and likewise a
``validation/main/boundary/map`` column (Boundary AP, --eval-boundary).
"""
import argparse
import datetime
import json
import os
import os.path as osp

KEYS = ['name', 'elapsed_time', 'last_time', 'git_hash', 'hostname', 'model', 'initializer', 'lr',
        'epoch', 'iteration', 'eval_result', 'validation/main/map']


BBOX_KEY = 'validation/main/bbox/map'
BOUNDARY_KEY = 'validation/main/boundary/map'


def log_has_key(logs_dir, name, key):
    try:
        with open(osp.join(logs_dir, name, 'log')) as f:
            return any(key in entry for entry in json.load(f))
    except Exception:
        return False


def seconds_to_string(seconds):
    seconds = int(round(seconds))
    minutes, seconds = seconds // 60, seconds % 60
    hours, minutes = minutes // 60, minutes % 60
    return '{:02d}:{:02d}:{:02d}'.format(hours, minutes, seconds)


def summarize_log(logs_dir, name, keys, target_key, objective, now=None):
    import pandas
    import yaml
    try:
        with open(osp.join(logs_dir, name, 'params.yaml')) as f:
            params = yaml.safe_load(f)
    except Exception:
        return None, None, osp.join(logs_dir, name)

    try:
        with open(osp.join(logs_dir, name, 'log')) as f:
            df = pandas.DataFrame(json.load(f))
    except Exception:
        df = None

    try:
        idx = df[target_key].idxmin() if objective == 'min' else df[target_key].idxmax()
    except Exception:
        idx = None
    if idx is not None and idx != idx:       # NaN: no entry holds the key
        idx = None

    eval_result = None
    eval_result_file = osp.join(logs_dir, name, 'snapshot_model.npz.eval_result.yaml')
    if osp.exists(eval_result_file):
        with open(eval_result_file) as f:
            eval_result = yaml.safe_load(f)

    dfi = df.loc[idx] if idx is not None else None
    row = []
    is_active = True
    for key in keys:
        if key == 'name':
            row.append(name)
        elif key == 'elapsed_time':
            row.append('<none>' if dfi is None else seconds_to_string(df[key].max()))
        elif key in ('epoch', 'iteration'):
            value = '<none>' if dfi is None else '%d' % dfi[key]
            row.append('<none>' if df is None else '%s /%d' % (value, df[key].max()))
        elif key.endswith('/loss'):
            value = '<none>' if dfi is None else '%.3f' % dfi[key]
            row.append('<none>' if df is None else
                       '%.3f< %s <%.3f' % (df[key].min(), value, df[key].max()))
        elif key.endswith('/map'):
            min_value = max_value = '<none>'
            value = '<none>' if dfi is None or key not in dfi else '%.3f' % dfi[key]
            if objective == 'max':
                if df is not None and key in df:
                    min_value = '%.3f' % df[key].min()
                row.append('%s< %s' % (min_value, value))
            else:
                if df is not None and key in df:
                    max_value = '%.3f' % df[key].max()
                row.append('%s <%s' % (value, max_value))
        elif key == 'last_time':
            value = '<none>'
            if df is not None and params.get('timestamp'):
                end = datetime.datetime.fromisoformat(params['timestamp']) + \
                    datetime.timedelta(seconds=float(df['elapsed_time'].max()))
                ago = (now or datetime.datetime.now()) - end
                if ago > datetime.timedelta(minutes=10):
                    is_active = False
                ago = max(datetime.timedelta(seconds=0), ago)
                value = '- %s' % seconds_to_string(ago.total_seconds())
            row.append(value)
        elif key == 'eval_result':
            row.append(None if eval_result is None else '%.3f' % eval_result['validation/main/map'])
        elif key in params:
            row.append(params[key])
        elif dfi is not None and key in dfi:
            row.append(dfi[key])
        else:
            row.append('<none>')
    return row, is_active, None


def summarize_logs(logs_dir, keys=KEYS, target_key='validation/main/map', objective='max'):
    import tabulate
    assert objective in ('min', 'max')
    assert target_key in keys
    for optional in (BBOX_KEY, BOUNDARY_KEY):
        if optional not in keys and any(log_has_key(logs_dir, name, optional)
                                        for name in sorted(os.listdir(logs_dir))):
            keys = list(keys) + [optional]
    rows, ignored = [], []
    for name in sorted(os.listdir(logs_dir)):
        row, _, ignored_dir = summarize_log(logs_dir, name, keys, target_key, objective)
        if ignored_dir:
            ignored.append(ignored_dir)
        else:
            rows.append(row)
    print('logs_dir: {}\n'.format(osp.abspath(logs_dir)))
    rows = sorted(rows, key=lambda x: x[0], reverse=True)
    print(tabulate.tabulate(rows, headers=keys, floatfmt='.3f', tablefmt='simple',
                            numalign='center', stralign='center', showindex=True,
                            disable_numparse=True))
    if ignored:
        print('Ignored logs:')
        for d in ignored:
            print('  - %s' % d)
    return rows, ignored


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('logs_dir', nargs='?', default='logs')
    args = ap.parse_args()
    summarize_logs(args.logs_dir)


if __name__ == '__main__':
    main()
