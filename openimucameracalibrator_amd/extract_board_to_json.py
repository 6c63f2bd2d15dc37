"""python -m openimucameracalibrator_amd.extract_board_to_json: the reference's applications/extract_board_to_json.cc
(board_extractor.BoardExtractor, radon board and image folders only)."""
import sys

from .board_extractor import main

if __name__ == "__main__":
    sys.exit(main())
