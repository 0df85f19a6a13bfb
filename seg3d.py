"""`python seg3d.py train | predict ...`: 3D segmentation fine-tuning of the pre-trained PCRLv2 network; the implementation lives in
pcrlv2_amd/seg3d.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pcrlv2_amd.seg3d import main  # noqa: E402

if __name__ == '__main__':
    main(sys.argv[1:])
