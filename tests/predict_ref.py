"""Literal host restatements of the file-facing parts of /root/reference/predict.py and evaluate.py -- TEST INFRASTRUCTURE
ONLY (numpy + os; the product path is predict.py / predict_cli.py / evaluate.py of the package).  Fixture G19 was recorded
from the reference's own functions; tests/test_predict_cli_cpu.py checks these restatements against it, and the GPU tests
then use them as the expected value."""
import os

import numpy as np

EXTENSIONS = (".png", ".jpg", ".jpeg")


def output_path_ref(output, input_file):
    """predict.py:43-49 (get_output_path; the makedirs side effect is the caller's business here)."""
    base_name = os.path.splitext(os.path.basename(input_file))[0]
    if output is None:
        return os.path.join(os.path.dirname(input_file), f"{base_name}.png")
    return os.path.join(output, f"{base_name}.png")


def walk_ref(input_dir):
    """predict.py:61-68 (process_directory): os.walk order, suffix test on the lower-cased name."""
    image_files = []
    for root, _, files in os.walk(input_dir):
        for file in files:
            if file.lower().endswith(EXTENSIONS):
                image_files.append(os.path.join(root, file))
    return image_files


def grey_classes_ref(mask):
    """predict.py:52-58 (mask_to_image) and evaluate.py:150-154."""
    vis = np.zeros_like(mask, dtype=np.uint8)
    vis[mask == 0] = 0
    vis[mask == 1] = 128
    vis[mask == 2] = 255
    return vis


def grey_postprocessed_ref(mask):
    """evaluate.py:160-163: the post-processed multi-class map; class 1 is not named and stays 0."""
    vis = np.zeros_like(mask, dtype=np.uint8)
    vis[mask == 0] = 0
    vis[mask == 2] = 255
    return vis


def grey_binary_ref(mask):
    """evaluate.py:96-97 ((pred * 255).astype(uint8) of a 0/1 map) and :103-105 (0 -> 0, 1 -> 255) name the same coding."""
    vis = np.zeros_like(mask, dtype=np.uint8)
    vis[mask == 0] = 0
    vis[mask == 1] = 255
    return vis


def table_ref(fn):
    """The 256-entry table a grey coding amounts to."""
    return fn(np.arange(256, dtype=np.uint8))


def evaluate_dump_ref(batches_raw, batches_post, n_classes, postprocess):
    """The files evaluate(..., epoch_pred_dir=D) writes, as {relative path: uint8 [H,W] pixels}, in the order it writes
    them (evaluate.py:35-40, 88-105, 146-164).  batches_raw[k][i]: the raw prediction of sample i of batch k (class indices,
    or the 0/1 map of the binary head); batches_post[k][i]: the same after post-processing (read only when postprocess)."""
    files = {}
    batch_index = 0
    for k, raw in enumerate(batches_raw):
        batch_index += 1                                               # evaluate.py:86 / :144: incremented before the dump
        for i in range(len(raw)):
            name = f"pred_batch{batch_index}_sample{i}.png"
            files[name] = grey_binary_ref(np.asarray(raw[i])) if n_classes == 1 else grey_classes_ref(np.asarray(raw[i]))
            if postprocess:
                post = np.asarray(batches_post[k][i])
                files[os.path.join("postprocessed", name)] = (grey_binary_ref(post) if n_classes == 1
                                                              else grey_postprocessed_ref(post))
    return files
