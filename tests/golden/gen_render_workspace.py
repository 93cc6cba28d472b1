"""Writes render_workspace.json: the workspace totals (minus the MLP scratch) of the built library for
every case of render_host_cases.workspace_cases().  Run it at the commit whose totals are the
reference (from the repository root, after building):

    python tests/golden/gen_render_workspace.py [out.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), HERE]

import render_host_cases as C  # noqa: E402

if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'render_workspace.json')
    totals = C.workspace_totals()
    with open(out, 'w') as f:
        json.dump(totals, f, indent=0, sort_keys=True)
        f.write('\n')
    print(f'{len(totals)} totals -> {out}')
