"""Writes soccdpt_amd/utils/plasma_lut.py: the 256-entry plasma colour table of soccdpt_amd.utils.visualise as committed data.

    LUT[i] = round-half-even(255 * matplotlib._cm_listed._plasma_data[i]), stored B, G, R

OpenCV documents COLORMAP_PLASMA as matplotlib's plasma; cv2 itself is not a dependency, so byte parity with cv2.applyColorMap is checked only
where cv2 imports (tests/test_visualise_cpu.py).  Needs matplotlib; the package does not.

    python tools/make_plasma_lut.py
"""
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plasma_bgr() -> np.ndarray:
    from matplotlib._cm_listed import _plasma_data
    rgb = np.rint(255.0 * np.asarray(_plasma_data, dtype=np.float64)).astype(np.uint8)     # np.rint rounds half to even
    assert rgb.shape == (256, 3)
    return np.ascontiguousarray(rgb[:, ::-1])


def main():
    lut = plasma_bgr()
    assert tuple(lut[0, ::-1]) == (13, 8, 135) and tuple(lut[128, ::-1]) == (204, 71, 120) and tuple(lut[255, ::-1]) == (240, 249, 33)
    rows = [lut[i:i + 8].tobytes().hex() for i in range(0, 256, 8)]
    path = os.path.join(REPO, "soccdpt_amd", "utils", "plasma_lut.py")
    with open(path, "w") as f:
        f.write('"""Data, written by tools/make_plasma_lut.py: the plasma colour map as 256 x (B, G, R) bytes,\n'
                'round-half-even(255 * matplotlib._cm_listed._plasma_data[i]).  Do not edit by hand."""\n')
        f.write("PLASMA_BGR_HEX = (\n")
        for r in rows:
            f.write(f'    "{r}"\n')
        f.write(")\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
