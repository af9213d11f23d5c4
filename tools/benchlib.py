"""What the measurement scripts under tools/ share.  Imported as a sibling (``from benchlib import ...``): every bench_*.py is run as
``python tools/bench_x.py``, which puts tools/ first on sys.path."""
import json
import os

import numpy as np


def stat(xs):
    xs = [float(x) for x in xs]
    return {'median_ms': float(np.median(xs)), 'min_ms': min(xs), 'max_ms': max(xs)}


def sum_phases(events):
    """A (name, start event, end event) log (meshcore.Phase) -> {name: ms summed}; the events must have completed."""
    out = {}
    for name, e0, e1 in events:
        out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
    return out


def sum_kernels(profile_events):
    """hip.PROFILE_EVENTS, the brackets around single C-ABI launches -> {kernel: ms summed}."""
    return sum_phases((name, e0, e1) for name, _units, e0, e1, _flops in profile_events)


def extracted_mesh(net, dev, resolution, steps):
    """The mesh of a stage-1 network at (resolution, upsampling_steps) -> (vertices, faces), device tensors."""
    from psnerf_amd import hip
    from psnerf_amd.stage1.extracting import Extractor3D, iso_value
    ex = Extractor3D(net, device=dev, resolution0=resolution, upsampling_steps=steps)
    ex.generate_mesh()
    return hip.marching_cubes(ex.last_grid.contiguous(), iso_value(ex.threshold), 2 + ex.padding)


def write_profile(path, out):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(out))
