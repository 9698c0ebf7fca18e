"""CPU restatement of the reference's IMU front end, the checker of lk_decode_imu(_dev) / lk_imu_split_dev.

  read_imu_messages()  the fields of serialized sensor_msgs/Imu messages the front end reads (ROS1 serialisation: 312 bytes + the frame_id)
  Frontend.process()   RosInterface::imuCallBack (ros_interface.cc:194-219: the redundancy test against the previous message, kept or not;
                       the time check)
The IMU branch of syncPackage (ros_interface.cc:277-301) is the kin branch's rule word for word: kin_ref.sync_package / split_cursor.
"""
import numpy as np

import lk_pkg

lk_pkg.load()
from legkilo_amd import synth  # noqa: E402

MSG_DTYPE = np.dtype([("seq", "<u4"), ("sec", "<u4"), ("nsec", "<u4"), ("frame_id", "O"), ("gyr", "<f8", 3), ("acc", "<f8", 3)])


class BadLength(ValueError):
    pass


class BackwardsStamp(ValueError):
    pass


def read_imu_messages(buf, msg_off):
    """uint8 buffer + n + 1 offsets -> MSG_DTYPE array; BadLength (with the message's index as .index) when a message is not 312 + L bytes."""
    b = np.ascontiguousarray(buf, dtype=np.uint8)
    off = [int(v) for v in msg_off]
    out = np.zeros(len(off) - 1, dtype=MSG_DTYPE)
    for i, (o, e) in enumerate(zip(off[:-1], off[1:])):
        if e - o < synth.IMU_MSG_FIXED_BYTES:
            raise BadLength(f"message {i}: {e - o} bytes")
        seq, sec, nsec, L = (int(v) for v in b[o:o + 16].view("<u4"))
        if e - o != synth.IMU_MSG_FIXED_BYTES + L:
            err = BadLength(f"message {i}: {e - o} bytes, frame_id length {L}")
            err.index = i
            raise err
        out[i] = (seq, sec, nsec, bytes(b[o + 16:o + 16 + L]), b[o + L + synth.IMU_MSG_GYR:o + L + synth.IMU_MSG_GYR + 24].view("<f8"),
                  b[o + L + synth.IMU_MSG_ACC:o + L + synth.IMU_MSG_ACC + 24].view("<f8"))
    return out


class Frontend:
    """The per-message state the reference keeps: the callback's static previous message (linear_acceleration.z / angular_velocity.z) and
    the last kept stamp.  process() refuses a kept stamp older than the last kept one (the reference clears its cache there) and a
    malformed message, and then leaves the state as it was."""

    def __init__(self, redundancy=True):
        self.redundancy = bool(redundancy)
        self.last_acc_z = np.float64(0.0)   # static sensor_msgs::Imu last_imu_msg: zero-initialised
        self.last_gyr_z = np.float64(0.0)
        self.last_stamp = -np.inf

    def state(self):
        return dict(last_acc_z=float(self.last_acc_z), last_gyr_z=float(self.last_gyr_z), last_stamp=float(self.last_stamp))

    def process(self, buf, msg_off):
        ms = read_imu_messages(buf, msg_off)
        last_az, last_gz, last_t = self.last_acc_z, self.last_gyr_z, self.last_stamp
        out = []
        for m in ms:
            az, gz = np.float64(m["acc"][2]), np.float64(m["gyr"][2])
            if self.redundancy and az == last_az and gz == last_gz:   # ros_interface.cc:198-204: "previous" moves on a dropped message too
                last_az, last_gz = az, gz
                continue
            t = np.float64(m["sec"]) + 1e-9 * np.float64(m["nsec"])   # ros::Time::toSec
            if t < last_t:
                raise BackwardsStamp(f"stamp {t!r} after {last_t!r}")
            r = np.zeros((), dtype=synth.IMU_DTYPE)
            r["stamp"], r["acc"], r["gyr"] = t, m["acc"], m["gyr"]
            out.append(r)
            last_az, last_gz, last_t = az, gz, t
        self.last_acc_z, self.last_gyr_z, self.last_stamp = last_az, last_gz, last_t
        return np.array(out, dtype=synth.IMU_DTYPE) if out else np.zeros(0, dtype=synth.IMU_DTYPE)
