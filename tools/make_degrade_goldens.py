"""Generate tests/golden/degrade_kernels_golden.npz by IMPORTING the reference's own finetune/datasets/blur_kernels.py.

Runs only in the build container (needs /root/reference; the module needs numpy and scipy).  Its deterministic constructors are called
on a listed parameter grid - all seven blur-kernel families of finetune/configs/degradation.yaml, sizes 7 / 13 / 21, three parameter
sets each - and the inputs and outputs are stored; tests/test_degrade_cpu.py holds dove_amd.degrade.blur_kernel against them.  The sinc
family has a random constructor only: it is called with omega_range = [omega, omega], which its uniform draw returns exactly.
The file holds inputs and expected outputs only (no reference source text).
"""
import importlib.util
import os

import numpy as np

REF = "/root/reference/finetune/datasets/blur_kernels.py"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "degrade_kernels_golden.npz")

FAMILIES = ("iso", "aniso", "generalized_iso", "generalized_aniso", "plateau_iso", "plateau_aniso", "sinc")
SIZES = (7, 13, 21)
# sigma_x, sigma_y, angle, beta, omega
PARAMS = ((0.4, 2.7, -2.5, 0.6, 0.7), (1.3, 0.9, 0.3, 1.0, 1.9), (2.9, 1.7, 3.0, 1.8, 3.1))


def main():
    spec = importlib.util.spec_from_file_location("ref_blur_kernels", REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    fams, sizes, params, kernels = [], [], [], {}
    for fam in FAMILIES:
        for size in SIZES:
            for sx, sy, th, beta, omega in PARAMS:
                iso = fam.endswith("_iso") or fam == "iso"
                if fam in ("iso", "aniso"):
                    k = ref.bivariate_gaussian(size, sx, sy, th, is_isotropic=iso)
                elif fam.startswith("generalized"):
                    k = ref.bivariate_generalized_gaussian(size, sx, sy, th, beta, is_isotropic=iso)
                elif fam.startswith("plateau"):
                    k = ref.bivariate_plateau(size, sx, sy, th, beta, is_isotropic=iso)
                else:
                    k = ref.random_circular_lowpass_kernel([omega, omega], size)
                kernels[f"k{len(fams)}"] = np.asarray(k, dtype=np.float64)
                fams.append(fam)
                sizes.append(size)
                params.append((sx, sy, th, beta, omega))
    np.savez_compressed(OUT, families=np.array(fams), sizes=np.array(sizes), params=np.array(params, dtype=np.float64), **kernels)
    print("wrote", OUT, len(fams), "kernels,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
