"""Confusion matrices out of TensorBoard event files (reference utilities/read_summary_file.py):

    python -m hypelcnn_amd.utilities.read_summary_file <log dir> [steps...]

Every `validation_confusion` summary of the directory's event* files (all steps, or the listed ones) is written to
./<grandparent>_<parent>_s<step>.csv, then the statistics of stat_extractor are printed.  The files are decoded with
common/tb_events.py; a truncated or corrupt file is reported and what was read before the damage is kept (the
reference's DataLossError branch)."""
import glob
import os
import sys
from pathlib import Path

import numpy

from hypelcnn_amd.common import tb_events
from hypelcnn_amd.utilities.stat_extractor import extract_statistics_info, print_statistics_info


def confusion_from_tensor(tensor):
    """[C, C] DT_STRING tensor of decimal strings, row-major -> int matrix"""
    rows, cols = tensor["shape"]
    return numpy.asarray([int(s) for s in tensor["string_val"]], dtype=int).reshape(rows, cols)


def read_confusions(log_dir, steps=(), out_dir="."):
    """-> [(step, csv path, matrix)] of every validation_confusion found, CSVs written into out_dir"""
    found = []
    for event_path in sorted(glob.glob(os.path.join(log_dir, "event*"))):
        parent_dir = Path(event_path).resolve().parent
        try:
            for e in tb_events.read_events(event_path):
                if steps and e["step"] not in steps:
                    continue
                for val in e["values"]:
                    if val["tag"] == "validation_confusion" and "tensor" in val:
                        print("Step %i in %s" % (e["step"], event_path))
                        confusion_matrix = confusion_from_tensor(val["tensor"])
                        record_path = os.path.join(
                            out_dir, parent_dir.parent.name + "_" + parent_dir.name + "_s" + str(e["step"]) + ".csv")
                        print("Saving to file:", record_path)
                        numpy.savetxt(record_path, confusion_matrix, fmt="%d", delimiter=",")
                        found.append((e["step"], record_path, confusion_matrix))
        except ValueError as err:
            print("Error reading summary file: ", event_path, f"({err})")
    return found


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    found = read_confusions(argv[0], [int(s) for s in argv[1:]])
    print_statistics_info(extract_statistics_info([m for _, _, m in found]))
    return found


if __name__ == "__main__":
    main()
