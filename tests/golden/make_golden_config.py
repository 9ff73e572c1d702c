"""Write tests/golden/reference_training_config.json: the plugin sections of the reference's training config.

    python tests/golden/make_golden_config.py REFERENCE_CHECKOUT

Reads REFERENCE_CHECKOUT/configs/TriplaneTurbo_v1.yaml, replaces the OmegaConf interpolations (`${...}`) by a plain
scalar, and keeps the eight keys of its `system` section that instantiate the geometry, material, background and
second-stage renderer (tests/test_host_logic.py: test_reference_training_yaml_loads_into_the_plugins).  Only these
configuration values are written; the file is a data fixture.
"""
import json
import os
import re
import sys

import yaml

KEYS = ("geometry_type", "geometry", "material_type", "material", "background_type", "background",
        "renderer_2nd_type", "renderer_2nd")


def main(ref: str) -> None:
    txt = re.sub(r"\$\{[^}]*\}", "1", open(os.path.join(ref, "configs", "TriplaneTurbo_v1.yaml")).read())
    system = yaml.safe_load(txt)["system"]
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_training_config.json")
    with open(out, "w") as f:
        json.dump({k: system[k] for k in KEYS}, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
