"""`python luna_nodules.py extract | train | predict ...`: LUNA16 nodule classification on the pre-trained 3D encoder; the implementation lives in
pcrlv2_amd/luna_nodules.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pcrlv2_amd.luna_nodules import main  # noqa: E402

if __name__ == '__main__':
    main(sys.argv[1:])
