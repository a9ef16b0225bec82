"""What the GPU tests of the record's readers share (test_gpu_visualize.py, test_gpu_track.py): a host record placed on the device."""
import numpy as np

from odise_amd._lib import RECORD_TABLE_LEN


def upload_record(ctx, rec, hw, unaligned=False):
    """-> (buffer, ids [h,w], table): two views of one device record; unaligned: it starts one int32 past a 16-byte boundary."""
    h, w = hw
    off = 4 if unaligned else 0
    buf = ctx.to_device(np.concatenate([np.full(off // 4, -7, np.int32), rec]))
    return buf, buf.view((h, w), np.int32, off), buf.view((RECORD_TABLE_LEN,), np.int32, off + h * w * 4)
