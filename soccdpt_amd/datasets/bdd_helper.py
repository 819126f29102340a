"""Reader of one Bengaluru recording, with the module and class names, the constructor arguments and the frame dictionary of the reference's
`SOccDPT/datasets/bdd_helper.py` (`BengaluruDepthDatasetIterator`, :60-192):

    <recording>/rgb_img/<timestamp>.png, depth_img/<timestamp>.png, seg_img/<timestamp>.png
    <recording>/<recording id>.csv        one row per frame, the SECOND column is the timestamp

Everything here runs on the host and decodes with PIL: cv2 and pandas are not dependencies.  The reference's `cv2.cvtColor(frame, COLOR_BGR2RGB)` is a
flip of the channel axis, the CSV is read with the standard library (a value that parses as a number becomes one, as pandas would make it).  The
trajectory file (`<id>_traj.csv`) is not read: no training or evaluation path uses it.  The GPU side of a batch is bengaluru_driving_dataset.py."""
from __future__ import annotations

import csv
import os
from typing import Dict, List

import numpy as np
import yaml
from PIL import Image

DATASET_BASE = "~/Datasets/Depth_Dataset_Bengaluru"
DEFAULT_CALIB = os.path.join(DATASET_BASE, "calibration/pocoX3/calib.yaml")
DEFAULT_DATASET = os.path.join(DATASET_BASE, "1658384707877")

DISPARITY_MODES = {"L": np.uint8, "I;16": np.uint16, "F": np.float32}     # PIL mode -> what the decoded array holds


def rgb_seg_to_class(seg_frame: np.ndarray, color_2_class: Dict[tuple, int]) -> np.ndarray:
    """Host form of the class map (bdd_helper.py:10-25): zeros, then for every colour of the table in order its class where the pixel WITH CHANNELS 0
    AND 2 EXCHANGED equals it.  The batched GPU form is soccdpt_data_targets(class_map, flip=1) (csrc/batch_targets.hip)."""
    flipped = np.asarray(seg_frame)[:, :, ::-1]
    out = np.zeros(flipped.shape[:2], dtype=int)
    for color, cls in color_2_class.items():
        out[np.all(flipped == np.array(color), axis=-1)] = cls
    return out


def _number(text: str):
    for cast in (int, float):
        try:
            return cast(text)
        except ValueError:
            pass
    return text


def decode_color(path: str) -> np.ndarray:
    """PNG -> uint8 [H,W,3] with the channel axis flipped, as np.asarray(Image.open(path)) followed by cvtColor(COLOR_BGR2RGB) gives it: a contiguous
    array (the flip is paid here, in the decoding thread, not where the frame is staged for the upload)."""
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{path}: expected an 8-bit three-channel image, got mode {im.mode} with shape {a.shape}")
    return np.ascontiguousarray(a[:, :, ::-1])


def decode_disparity(path: str) -> np.ndarray:
    """PNG -> [H,W] of uint8 / uint16 / float32 exactly as stored (modes L, I;16 and F); anything else raises, naming the file and its mode."""
    with Image.open(path) as im:
        mode = im.mode
        if mode not in DISPARITY_MODES:
            raise ValueError(f"{path}: disparity images are one-channel PNGs of mode L, I;16 or F; this one has mode {mode}")
        a = np.asarray(im)
    if a.ndim != 2:
        raise ValueError(f"{path}: disparity images are two-dimensional; mode {mode} decoded to shape {a.shape}")
    return np.ascontiguousarray(a, dtype=DISPARITY_MODES[mode])


class BengaluruDepthDatasetIterator:
    def __init__(self, dataset_path: str = DEFAULT_DATASET, settings_doc: str = DEFAULT_CALIB, file_extension: str = ".png") -> None:
        self.dataset_path = os.path.expanduser(dataset_path)
        self.dataset_id = self.dataset_path.rstrip("/").split("/")[-1]
        self.rgb_img_folder = os.path.join(self.dataset_path, "rgb_img")
        self.depth_img_folder = os.path.join(self.dataset_path, "depth_img")
        self.seg_img_folder = os.path.join(self.dataset_path, "seg_img")
        self.csv_path = os.path.join(self.dataset_path, self.dataset_id + ".csv")
        self.traj_path = os.path.join(self.dataset_path, self.dataset_id + "_traj.csv")
        self.file_extension = file_extension

        self.settings_doc = os.path.expanduser(settings_doc)
        with open(self.settings_doc, "r") as stream:
            self.cam_settings = yaml.load(stream, Loader=yaml.FullLoader)
        s = self.cam_settings
        self.DistCoef = np.array([s["Camera.k1"], s["Camera.k2"], s["Camera.p1"], s["Camera.p2"], s.get("Camera.k3", 0)])
        self.intrinsic_matrix = np.array([[s["Camera.fx"], 0.0, s["Camera.cx"]], [0.0, s["Camera.fy"], s["Camera.cy"]], [0.0, 0.0, 1.0]])
        self.width = s["Camera.width"]
        self.height = s["Camera.height"]

        with open(self.csv_path, "r", newline="") as f:
            rows = list(csv.reader(f))
        assert rows and len(rows[0]) >= 2, f"{self.csv_path}: a header row and at least two columns (the second is the timestamp)"
        self.csv_columns: List[str] = rows[0]
        self.csv_dat: List[list] = [[_number(v) for v in r] for r in rows[1:] if r]
        self.traj_available = False      # <id>_traj.csv is not read here

    def __iter__(self):
        self.line_no = 0
        return self

    def __next__(self):
        if self.line_no >= self.__len__():
            raise StopIteration
        data = self[self.line_no]
        self.line_no += 1
        return data

    def __len__(self):
        return len(self.csv_dat)

    def frame_paths(self, key: int):
        """-> (csv row as {column: value}, rgb path, disparity path, label path) of frame `key`, with the reference's bounds and missing-file checks."""
        if key > len(self):
            raise IndexError("Out of bounds; key=", key)
        if key < 0 or key == len(self):      # what the reference's csv_dat.loc[key] raises for a label that is not in the index
            raise KeyError(key)
        csv_frame = dict(zip(self.csv_columns, self.csv_dat[key]))
        timestamp = str(int(self.csv_dat[key][1]))
        disparity_frame_path = os.path.join(self.depth_img_folder, timestamp + self.file_extension)
        seg_frame_path = os.path.join(self.seg_img_folder, timestamp + self.file_extension)
        rgb_frame_path = os.path.join(self.rgb_img_folder, timestamp + self.file_extension)
        assert os.path.isfile(disparity_frame_path), "File missing " + disparity_frame_path
        assert os.path.isfile(seg_frame_path), "File missing " + seg_frame_path
        assert os.path.isfile(rgb_frame_path), "File missing " + rgb_frame_path
        return csv_frame, rgb_frame_path, disparity_frame_path, seg_frame_path

    def read_frame(self, key: int) -> dict:
        """The frame dictionary: host arrays only, safe to call from a worker thread."""
        csv_frame, rgb_path, disparity_path, seg_path = self.frame_paths(key)
        frame = {
            "rgb_frame": decode_color(rgb_path),
            "disparity_frame": decode_disparity(disparity_path),
            "seg_frame": decode_color(seg_path),
            "csv_frame": csv_frame,
        }
        for column, value in csv_frame.items():
            frame[column] = value
        return frame

    def __getitem__(self, key):
        return self.read_frame(key)
