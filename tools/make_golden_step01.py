"""
Generate tests/golden/ref_step01_vectors.npz (+ .json) by running the REFERENCE's own
`specific_to_relative_humidity` of step_01_extract_deltas/Emon_convert_hus_to_hur.py (its Magnus formula, :16-21).

The module imports xarray and matplotlib at its top; neither is needed by that function, so they are replaced by empty
placeholder modules for the import (the way oracle/make_golden.py imports the reference's functions.py).  The
script's own work sits behind its `__main__` guard: importing it runs nothing.  Nothing of the reference is written
anywhere - the fixture holds inputs, outputs and result dtypes.

Cases: float64 QV / P / T, and float32 QV / T with a float64 P (what the script gets from float32 Emon files, whose
`plev` coordinate is float64), temperatures from 180 K to 330 K.

usage:  python tools/make_golden_step01.py REFERENCE_DIR
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, '..', 'tests', 'golden')


def import_reference_emon(ref_dir):
    for name in ['xarray', 'matplotlib', 'matplotlib.pyplot']:
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules['matplotlib'].pyplot = sys.modules['matplotlib.pyplot']
    sys.dont_write_bytecode = True
    path = os.path.join(ref_dir, 'step_01_extract_deltas', 'Emon_convert_hus_to_hur.py')
    spec = importlib.util.spec_from_file_location('ref_emon_convert_hus_to_hur', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref_dir):
    M = import_reference_emon(ref_dir)
    rng = np.random.default_rng(20261016)
    n = 4096
    T = np.concatenate([np.linspace(180., 330., n // 2), rng.uniform(180., 330., n - n // 2)])
    P = rng.choice(np.array([100000., 92500., 85000., 70000., 60000., 50000., 40000., 30000., 25000., 20000., 15000.,
                             10000., 7000., 5000., 3000., 2000., 1000., 500., 100.]), n)
    QV = np.exp(rng.uniform(np.log(1e-7), np.log(3e-2), n))
    out, meta = {}, {'source': 'step_01_extract_deltas/Emon_convert_hus_to_hur.py:16-21 specific_to_relative_humidity(QV, P, T)',
                     'numpy': np.__version__, 'cases': {}}
    for tag, dt in (('f64', np.float64), ('f32', np.float32)):
        qv, t = QV.astype(dt), T.astype(dt)
        rh = M.specific_to_relative_humidity(qv, P, t)
        out['%s_QV' % tag], out['%s_P' % tag], out['%s_T' % tag], out['%s_RH' % tag] = qv, P, t, rh
        meta['cases'][tag] = dict(QV=str(qv.dtype), P=str(P.dtype), T=str(t.dtype), RH=str(rh.dtype), n=n)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, 'ref_step01_vectors.npz'), **out)
    with open(os.path.join(OUT, 'ref_step01_vectors.json'), 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(meta['cases']))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
