"""A minimal safetensors writer for tests: header length, JSON header, raw data. Takes (dtype name, numpy array of the raw storage type)."""
import json
import struct

import numpy as np


def write_safetensors(path, tensors):
    """tensors: name -> (dtype string such as "BF16" / "F32" / "U32", shape, numpy array whose bytes are the data)."""
    header, blobs, off = {}, [], 0
    for name, (dtype, shape, arr) in tensors.items():
        raw = np.ascontiguousarray(arr).tobytes()
        header[name] = {"dtype": dtype, "shape": list(shape), "data_offsets": [off, off + len(raw)]}
        blobs.append(raw)
        off += len(raw)
    js = json.dumps(header).encode()
    js += b" " * (-len(js) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(js)))
        f.write(js)
        for b in blobs:
            f.write(b)
