"""Write tests/golden/reference_mesh_renderer_config.json: the first renderer of the reference's training config.

    python tests/golden/make_golden_mesh_renderer_config.py REFERENCE_CHECKOUT

Reads REFERENCE_CHECKOUT/configs/TriplaneTurbo_v1.yaml, replaces the OmegaConf interpolations (`${...}`) by a plain
scalar (make_golden_config.py does the same), and keeps `system.renderer_type` and `system.renderer`
(tests/test_raster_host.py).  Only these configuration values are written; the file is a data fixture.
"""
import json
import os
import re
import sys

import yaml

KEYS = ("renderer_type", "renderer")


def main(ref: str) -> None:
    txt = re.sub(r"\$\{[^}]*\}", "1", open(os.path.join(ref, "configs", "TriplaneTurbo_v1.yaml")).read())
    system = yaml.safe_load(txt)["system"]
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_mesh_renderer_config.json")
    with open(out, "w") as f:
        json.dump({k: system[k] for k in KEYS}, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
