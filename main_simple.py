"""`python main_simple.py ...` exactly as in the reference README; forwards to linkteller_amd.main_simple."""
from linkteller_amd.main_simple import main

if __name__ == "__main__":
    main()
