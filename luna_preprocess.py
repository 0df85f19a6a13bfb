"""`python luna_preprocess.py --data LUNA16 --save out` like the reference (luna_preprocess.py); the implementation lives in
pcrlv2_amd/luna_prep.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pcrlv2_amd.luna_prep import main  # noqa: E402

if __name__ == '__main__':
    main(sys.argv[1:])
