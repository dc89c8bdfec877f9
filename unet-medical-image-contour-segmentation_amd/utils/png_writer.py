"""Background PNG output shared by `python -m unet_amd.predict` and evaluate(epoch_pred_dir=...): grey uint8 [H,W] arrays
are encoded by a thread pool while the device works on the next batch, and the files are committed in a stated order.

    w = OrderedPngWriter(workers=8)
    w.submit(order, path, array)      # encode in the pool; the file is written once every smaller `order` has been settled
    w.skip(order)                     # nothing will come for this position (an input that failed to decode)
    w.close()                         # returns when every submitted file is on disk; re-raises the first write error

The order matters where two results share a path (predict.py writes every mask flat into --output as <stem>.png, so equal
stems collide and the later input wins): committing in input order keeps the reference's winner whatever order the
batches finished in.  Positions start at 0 and every position must be submitted or skipped exactly once."""
from __future__ import annotations

import io
import os
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Tuple

import numpy as np


def encode_png(array: np.ndarray) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(array, dtype=np.uint8)).save(buf, format="PNG")      # mode L, as Image.fromarray(uint8 2-D)
    return buf.getvalue()


class OrderedPngWriter:
    def __init__(self, workers: int = 8, pool: Optional[ThreadPoolExecutor] = None):
        self._own = pool is None
        self._pool = pool if pool is not None else ThreadPoolExecutor(max_workers=max(1, int(workers)),
                                                                       thread_name_prefix="png")
        self._lock = threading.Lock()
        self._ready: Dict[int, Optional[Tuple[str, bytes]]] = {}
        self._next = 0
        self._futures: List = []
        self._error: Optional[BaseException] = None
        self.written: List[str] = []

    def _settle(self, order: int, item) -> None:
        with self._lock:
            self._ready[order] = item
            while self._next in self._ready:
                it = self._ready.pop(self._next)
                self._next += 1
                if it is None or self._error is not None:
                    continue
                try:
                    with open(it[0], "wb") as f:
                        f.write(it[1])
                    self.written.append(it[0])
                except BaseException as e:                              # reported by close()
                    self._error = e

    def _encode(self, order: int, path: str, array: np.ndarray) -> None:
        try:
            item = (path, encode_png(array))
        except BaseException as e:
            with self._lock:
                self._error = self._error or e
            item = None
        self._settle(order, item)

    def submit(self, order: int, path, array: np.ndarray) -> None:
        self._futures.append(self._pool.submit(self._encode, int(order), os.fspath(path), array))

    def skip(self, order: int) -> None:
        self._settle(int(order), None)

    def close(self) -> List[str]:
        for f in self._futures:
            f.result()
        self._futures = []
        if self._own:
            self._pool.shutdown(wait=True)
        if self._error is not None:
            raise self._error
        if self._ready:
            raise RuntimeError(f"OrderedPngWriter: positions {sorted(self._ready)} wait for position {self._next}, which was never settled")
        return self.written
